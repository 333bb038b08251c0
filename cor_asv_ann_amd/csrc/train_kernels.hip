// Memory-bound kernels of the train step (kt:195 `train_on_batch`): everything of forward / backward /
// update that is not a contraction.  All sequence tensors of the train step are TIME-MAJOR,
// [t][b][feature], so that one time step is a contiguous [B][F] slab (a GEMM operand) and a whole
// sequence is a [T*B][F] matrix (operand of the batched weight-gradient GEMMs).
#include "train_kernels.h"
#include "attn_bwd.h"
#include "alt_order.h"
#include <math.h>

namespace casv {

__device__ __forceinline__ float wsum(float v) { return wave_butterfly(v, [](float a, float b) { return a + b; }); }

// ---- transpose: dst[c][r] = src[r][c] (32x32 tiles through LDS) ----
__global__ void transpose_kernel(const float* __restrict__ src, int rows, int cols, long long ld_src,
                                 float* __restrict__ dst, long long ld_dst) {
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 256 threads: 8 rows per pass
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? src[(long long)r * ld_src + c] : 0.0f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows) dst[(long long)c * ld_dst + r] = tile[tx][i];
    }
}
void launch_transpose(const float* src, int rows, int cols, long long ld_src, float* dst, long long ld_dst, hipStream_t st) {
    hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, st, src, rows, cols, ld_src, dst, ld_dst);
}

// ---- embedding rows, time-major output: out[(t*B+b)][:] = sum_a val * E[idx[b][t][a]] ----
__global__ void embed_tm_kernel(const float* __restrict__ E, const int* __restrict__ idx, const float* __restrict__ val,
                                float* __restrict__ out, int B, int T, int A, int V, int W) {
    const int t = blockIdx.x / B, b = blockIdx.x % B;
    const long long in = ((long long)b * T + t) * A;
    for (int w = threadIdx.x * 4; w < W; w += blockDim.x * 4) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < A; ++k) {
            const int i = idx[in + k];
            if (i < 0 || i >= V) continue;
            const float c = val ? val[in + k] : 1.0f;
            const float4 e = *reinterpret_cast<const float4*>(E + (long long)i * W + w);
            acc.x += c * e.x; acc.y += c * e.y; acc.z += c * e.z; acc.w += c * e.w;
        }
        *reinterpret_cast<float4*>(out + ((long long)t * B + b) * W + w) = acc;
    }
}
void launch_embed_tm(const float* E, const int* idx, const float* val, float* out, int B, int T, int A, int V, int W, hipStream_t st) {
    hipLaunchKernelGGL(embed_tm_kernel, dim3(B * T), dim3(128), 0, st, E, idx, val, out, B, T, A, V, W);
}

// dE[idx] += val * dX[(t*B+b)]   (float atomics: rows of frequent characters collide)
__global__ void embed_scatter_kernel(float* __restrict__ dE, const int* __restrict__ idx, const float* __restrict__ val,
                                     const float* __restrict__ dX, long long ld_dx, int B, int T, int A, int V, int W) {
    const int t = blockIdx.x / B, b = blockIdx.x % B;
    const long long in = ((long long)b * T + t) * A;
    const float* src = dX + ((long long)t * B + b) * ld_dx;
    for (int k = 0; k < A; ++k) {
        const int i = idx[in + k];
        if (i < 0 || i >= V) continue;
        const float c = val ? val[in + k] : 1.0f;
        for (int w = threadIdx.x; w < W; w += blockDim.x) atomicAdd(dE + (long long)i * W + w, c * src[w]);
    }
}
void launch_embed_scatter(float* dE, const int* idx, const float* val, const float* dX, long long ld_dx, int B, int T, int A,
                          int V, int W, hipStream_t st) {
    hipLaunchKernelGGL(embed_scatter_kernel, dim3(B * T), dim3(128), 0, st, dE, idx, val, dX, ld_dx, B, T, A, V, W);
}

// ---- ordered sums (the train step's "deterministic" option) ----
// *acc += parts[0] + parts[1] + ... + parts[n-1]: one workgroup, strided partial sums and a fixed tree -- the same order every run
__global__ __launch_bounds__(256) void ordered_sum_kernel(const double* __restrict__ parts, int n, double* __restrict__ acc) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += parts[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) *acc += red[0];
}
static void ordered_sum(const double* parts, int n, double* acc, hipStream_t st) {
    hipLaunchKernelGGL(ordered_sum_kernel, dim3(1), dim3(256), 0, st, parts, n, acc);
}

// dE[v][w] += sum over the rows that use character v, in row order, of val * dX[row][w]: the embedding gradient as per-character
// segments (seg_off [V+1], seg_pos = positions (b*T + t)*A + k of the index array, sorted by character, within one by (t, b, k))
__global__ void embed_segments_kernel(float* __restrict__ dE, const int* __restrict__ seg_off, const int* __restrict__ seg_pos,
                                      const float* __restrict__ val, const float* __restrict__ dX, long long ld_dx, int B, int T, int A, int W) {
    const int v = blockIdx.x, p0 = seg_off[v], p1 = seg_off[v + 1];
    if (p0 == p1) return;
    for (int w = threadIdx.x; w < W; w += blockDim.x) {
        float s = 0.f;
        for (int q = p0; q < p1; ++q) {
            const int pos = seg_pos[q], bt = pos / A, b = bt / T, t = bt % T;
            s += (val ? val[pos] : 1.0f) * dX[((long long)t * B + b) * ld_dx + w];
        }
        dE[(long long)v * W + w] += s;
    }
}
void launch_embed_segments(float* dE, const int* seg_off, const int* seg_pos, const float* val, const float* dX, long long ld_dx,
                           int B, int T, int A, int V, int W, hipStream_t st) {
    hipLaunchKernelGGL(embed_segments_kernel, dim3(V), dim3(128), 0, st, dE, seg_off, seg_pos, val, dX, ld_dx, B, T, A, W);
}

// ---- out[r][f] = in[r][f] * mask[f] (+ add[r][f]) : time-constant dropout masks (seq2seq.py:298,367) ----
__global__ void mul_mask_kernel(const float* __restrict__ in, long long ld_in, const float* __restrict__ mask,
                                float* __restrict__ out, long long ld_out, long long rows, int F) {
    const long long n = rows * F;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / F; const int f = (int)(i % F);
        out[r * ld_out + f] = in[r * ld_in + f] * (mask ? mask[f] : 1.0f);
    }
}
void launch_mul_mask(const float* in, long long ld_in, const float* mask, float* out, long long ld_out, long long rows, int F, hipStream_t st) {
    const long long n = rows * F;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(mul_mask_kernel, dim3(blocks), dim3(256), 0, st, in, ld_in, mask, out, ld_out, rows, F);
}

__global__ void add_mul_mask_kernel(const float* __restrict__ a, long long lda, const float* __restrict__ b, long long ldb,
                                    const float* __restrict__ mask, float* __restrict__ out, long long ld_out, long long rows, int F) {
    const long long n = rows * F;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / F; const int f = (int)(i % F);
        out[r * ld_out + f] = (a[r * lda + f] + b[r * ldb + f]) * (mask ? mask[f] : 1.0f);
    }
}
void launch_add_mul_mask(const float* a, long long lda, const float* b, long long ldb, const float* mask, float* out, long long ld_out,
                         long long rows, int F, hipStream_t st) {
    const long long n = rows * F;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(add_mul_mask_kernel, dim3(blocks), dim3(256), 0, st, a, lda, b, ldb, mask, out, ld_out, rows, F);
}
// ---- out[r * N + n][f] = in[r][f]: every row N times in a row (casv_score_candidates: a source's final states for its N candidates) ----
__global__ void repeat_rows_kernel(const float* __restrict__ in, float* __restrict__ out, long long rows, int N, int F) {
    const long long n = rows * N * F;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / F; const int f = (int)(i % F);
        out[i] = in[(r / N) * F + f];
    }
}
void launch_repeat_rows(const float* in, float* out, long long rows, int N, int F, hipStream_t st) {
    const long long n = rows * N * F;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(repeat_rows_kernel, dim3(blocks), dim3(256), 0, st, in, out, rows, N, F);
}
__global__ void tanh_bwd_kernel(float* __restrict__ dy, const float* __restrict__ y, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dy[i] *= 1.0f - y[i] * y[i];
}
void launch_tanh_bwd(float* dy, const float* y, long long n, hipStream_t st) {
    const int blocks = (int)std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(tanh_bwd_kernel, dim3(blocks), dim3(256), 0, st, dy, y, n);
}

// ---- out[(t*B+b)][f] = in[(t*B+b)][f] * mask[b][f]: per-sample, time-constant mask ----
__global__ void mul_rowmask_kernel(const float* __restrict__ in, long long ld_in, const float* __restrict__ mask, long long ld_mask,
                                   float* __restrict__ out, long long ld_out, long long rows, int B, int F) {
    const long long n = rows * F;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / F; const int f = (int)(i % F);
        out[r * ld_out + f] = in[r * ld_in + f] * (mask ? mask[(r % B) * ld_mask + f] : 1.0f);
    }
}
void launch_mul_rowmask(const float* in, long long ld_in, const float* mask, long long ld_mask, float* out, long long ld_out,
                        long long rows, int B, int F, hipStream_t st) {
    const long long n = rows * F;
    hipLaunchKernelGGL(mul_rowmask_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 4096)), dim3(256), 0, st, in, ld_in, mask,
                       ld_mask, out, ld_out, rows, B, F);
}

// ---- softmax + weighted categorical cross-entropy (Keras), dlogits in place ----
// One wave per row, a workgroup's waves walk the rows with the grid's stride; the loss terms are summed per wave and per
// workgroup first (float64) and reach the accumulator as ONE atomic per workgroup: 52 224 adds to a single address -- one per
// row -- were 0.63 ms of the step (profiles/r02_train_kernel_stats.csv: softmax_ce_kernel), every one serialised behind the
// others at the memory side.
template <bool ORDERED>        // ORDERED: the workgroup's sum goes to parts[blockIdx.x] (ordered_sum adds them)
__global__ __launch_bounds__(256) void softmax_ce_kernel(float* __restrict__ logits, const int* __restrict__ target,
                                                         const float* __restrict__ weight, long long rows, int B, int U, int V,
                                                         int Vp, float inv_count, double* __restrict__ loss, int want_grad) {
    __shared__ double part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double mine = 0.0;
    for (long long r = blockIdx.x * 4LL + wave; r < rows; r += 4LL * gridDim.x) {
        float* x = logits + r * Vp;
        float m = -INFINITY;
        for (int v = lane; v < V; v += 64) m = fmaxf(m, x[v]);
        m = wave_butterfly(m, [](float a, float b) { return fmaxf(a, b); });
        float sum = 0.f;
        for (int v = lane; v < V; v += 64) sum += expf(x[v] - m);
        sum = wsum(sum);
        const long long src = (r % B) * U + r / B;        // row r = t*B + b  <-  (b, t) of the caller's (B,U) arrays
        const int tg = target[src];
        const float wgt = weight[src];
        float pt = 0.f;
        if (tg >= 0 && tg < V) pt = expf(x[tg] - m) / sum;
        const bool ok = tg >= 0 && pt > 1e-7f && pt < 1.0f - 1e-7f;      // tf.clip_by_value passes gradient inside only
        if (tg >= 0) {
            const float pc = fminf(fmaxf(pt, 1e-7f), 1.0f - 1e-7f);
            mine += (double)(-logf(pc) * wgt * inv_count);               // (the same value in every lane)
        }
        if (want_grad) {
            const float sc = ok ? wgt * inv_count : 0.0f;
            for (int v = lane; v < Vp; v += 64) {
                float gvl = 0.f;
                if (v < V) gvl = (expf(x[v] - m) / sum - (v == tg ? 1.0f : 0.0f)) * sc;
                x[v] = gvl;
            }
        }
    }
    if (lane == 0) part[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s4 = part[0] + part[1] + part[2] + part[3];
        if (ORDERED) loss[blockIdx.x] = s4;
        else if (s4 != 0.0) atomicAdd(loss, s4);
    }
}
void launch_softmax_ce(float* logits, const int* target, const float* weight, int B, int U, int V, int Vp, float inv_count,
                       double* loss, int want_grad, hipStream_t st, double* parts) {
    const long long rows = (long long)B * U;
    const long long wgs = std::min<long long>((rows + 3) / 4, 2048);
    if (parts) {
        hipLaunchKernelGGL(softmax_ce_kernel<true>, dim3((unsigned)wgs), dim3(256), 0, st, logits, target, weight, rows, B, U, V,
                           Vp, inv_count, parts, want_grad);
        ordered_sum(parts, (int)wgs, loss, st);
        return;
    }
    hipLaunchKernelGGL(softmax_ce_kernel<false>, dim3((unsigned)wgs), dim3(256), 0, st, logits, target, weight, rows, B, U, V,
                       Vp, inv_count, loss, want_grad);
}

// ---- the same head on soft targets (casv_train_step_soft): K (index, mass) slots per row instead of one index ----
// One wave per row and m, sum and p_v formed as softmax_ce_kernel forms them.  Lane k holds slot k (K <= 64; index -1 = empty): its
// p[i_k], its loss term q_k * -log(clip(p)) and q_k * ok_k, ok_k the hard head's strict rule for that entry; the terms and
// S = sum q_k ok_k are summed across the wave by the butterfly (one order whatever the launch shape).  With one slot (i, 1.0) every
// value has the bits of softmax_ce_kernel's for target i.  dlogit[v] = (p_v * S - q ok of the slot with i_k == v) * w * inv_count:
// the dense pass looks the slots up, lane k's pair broadcast to the wave in the order of k (the indices of a row are distinct, so
// at most one matches), outside every divergent branch -- one store per element, by the lane that owns it; no LDS, no atomics.
// Columns [V, Vp) are never read and written as zeros.
template <bool ORDERED>
__global__ __launch_bounds__(256) void soft_ce_kernel(float* __restrict__ logits, const int* __restrict__ soft_idx,
                                                      const float* __restrict__ soft_q, const float* __restrict__ weight, long long rows,
                                                      int B, int U, int V, int Vp, int K, float inv_count, double* __restrict__ loss,
                                                      int want_grad) {
    __shared__ double part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double mine = 0.0;
    for (long long r = blockIdx.x * 4LL + wave; r < rows; r += 4LL * gridDim.x) {
        float* x = logits + r * Vp;
        float m = -INFINITY;
        for (int v = lane; v < V; v += 64) m = fmaxf(m, x[v]);
        m = wave_butterfly(m, [](float a, float b) { return fmaxf(a, b); });
        float sum = 0.f;
        for (int v = lane; v < V; v += 64) sum += expf(x[v] - m);
        sum = wsum(sum);
        const long long src = (r % B) * U + r / B;        // row r = t*B + b  <-  (b, t) of the caller's (B,U,K) arrays
        const float wgt = weight[src];
        int ik = -1;
        float qk = 0.f;
        if (lane < K) { ik = soft_idx[src * K + lane]; qk = soft_q[src * K + lane]; }
        const bool slot = ik >= 0 && ik < V;
        if (!slot) ik = -1;
        float term = 0.f, qok = 0.f;
        if (slot) {
            const float pk = expf(x[ik] - m) / sum;
            term = qk * -logf(fminf(fmaxf(pk, 1e-7f), 1.0f - 1e-7f));
            if (pk > 1e-7f && pk < 1.0f - 1e-7f) qok = qk;               // tf.clip_by_value passes gradient inside only
        }
        const float terms = wsum(term), S = wsum(qok);
        if (__ballot(slot) != 0ull) mine += (double)(terms * wgt * inv_count);      // (the same value in every lane)
        if (want_grad) {
            const float sc = wgt * inv_count;
            for (int v0 = 0; v0 < Vp; v0 += 64) {
                const int v = v0 + lane;
                float sub = 0.f;
                for (int k = 0; k < K; ++k) {
                    const int i = __builtin_amdgcn_readlane(ik, k);
                    const float q = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(qok), k));
                    sub = i == v ? q : sub;
                }
                float gvl = 0.f;
                if (v < V) gvl = (expf(x[v] - m) / sum * S - sub) * sc;
                if (v < Vp) x[v] = gvl;
            }
        }
    }
    if (lane == 0) part[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s4 = part[0] + part[1] + part[2] + part[3];
        if (ORDERED) loss[blockIdx.x] = s4;
        else if (s4 != 0.0) atomicAdd(loss, s4);
    }
}
void launch_soft_ce(float* logits, const int* soft_idx, const float* soft_q, const float* weight, int B, int U, int V, int Vp, int K,
                    float inv_count, double* loss, int want_grad, hipStream_t st, double* parts) {
    const long long rows = (long long)B * U;
    const long long wgs = std::min<long long>((rows + 3) / 4, 2048);
    if (parts) {
        hipLaunchKernelGGL(soft_ce_kernel<true>, dim3((unsigned)wgs), dim3(256), 0, st, logits, soft_idx, soft_q, weight, rows, B, U, V,
                           Vp, K, inv_count, parts, want_grad);
        ordered_sum(parts, (int)wgs, loss, st);
        return;
    }
    hipLaunchKernelGGL(soft_ce_kernel<false>, dim3((unsigned)wgs), dim3(256), 0, st, logits, soft_idx, soft_q, weight, rows, B, U, V,
                       Vp, K, inv_count, loss, want_grad);
}

// ---- scoring head (casv_score_targets, kt:407 / s2s:491-497 without the clip): log-probability, argmax and rank per row ----
// One wave per row, as softmax_ce_kernel; two passes over the row's first V columns (the padding columns [V, Vp) are never read):
// the maximum and the NaN test, then the exponentials' sum, the lowest index of the maximum and the count of entries above the
// target's.  Nothing is written back into the logits, no probability is formed: logp = (x[t] - m) - log(sum exp(x - m)).
// The results go out in the caller's (B,U) order, src = b * U + u of row r = u * B + b.
__global__ __launch_bounds__(256) void score_rows_kernel(const float* __restrict__ logits, const int* __restrict__ target, long long rows,
                                                         int B, int U, int V, int Vp, float* __restrict__ logp, int* __restrict__ best,
                                                         int* __restrict__ rank) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long r = blockIdx.x * 4LL + wave; r < rows; r += 4LL * gridDim.x) {
        const float* x = logits + r * Vp;
        float m = -INFINITY;
        int nan = 0;
        for (int v = lane; v < V; v += 64) { const float xv = x[v]; nan |= xv != xv; m = fmaxf(m, xv); }      // (fmaxf passes a NaN by)
        m = wave_butterfly(m, [](float a, float b) { return fmaxf(a, b); });
        nan = wave_butterfly(nan, [](int a, int b) { return a | b; });
        const bool valid = !nan && m > -INFINITY && m < INFINITY;
        const long long src = (r % B) * U + r / B;
        const int tg = target[src];
        const bool scored = tg >= 0 && tg < V;
        const float xt = scored ? x[tg] : 0.f;
        float sum = 0.f;
        int first = V, above = 0;
        for (int v = lane; v < V; v += 64) {
            const float xv = x[v];
            sum += expf(xv - m);
            if (xv == m) first = min(first, v);
            above += xv > xt;
        }
        sum = wsum(sum);
        first = wave_butterfly(first, [](int a, int b) { return min(a, b); });
        above = wave_butterfly(above, [](int a, int b) { return a + b; });
        if (lane == 0) {
            logp[src] = !valid ? __builtin_nanf("") : scored ? (xt - m) - logf(sum) : 0.f;
            best[src] = valid ? first : -1;
            rank[src] = valid && scored ? above : -1;
        }
    }
}
void launch_score_rows(const float* logits, const int* target, int B, int U, int V, int Vp, float* logp, int* best, int* rank,
                       hipStream_t st) {
    const long long rows = (long long)B * U;
    const long long wgs = std::min<long long>((rows + 3) / 4, 2048);
    hipLaunchKernelGGL(score_rows_kernel, dim3((unsigned)wgs), dim3(256), 0, st, logits, target, rows, B, U, V, Vp, logp, best, rank);
}

// ---- minimum-risk head (casv_train_step_risk): N costed candidates per group, the coefficients formed between forward and backward ----
// Three launches on the logits [U*B][Vp]: score_rows_kernel leaves logp [B][U] (its best / rank are by-products nobody reads);
// risk_weight_kernel turns them into one coefficient per line; risk_grad_kernel writes dL/dlogits in place.
__device__ __forceinline__ double readlane_d(const double v, const int k) {      // k wave-uniform
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}
// One wave per group g, lane i < N holds candidate i = line g * N + i: its cost (negative: not a member), its own serial float64
// sum s over u ascending of (double)(w * logp) -- a float32 product -- at the positions the loss heads score (0 <= t < V, w != 0).
// Max, Z and the risk are taken across the lanes by serial readlane loops in i, outside every divergent branch: one order
// whatever the launch shape, no LDS, no atomics.  Writes coef [B] (float32), q [B], risk [G] (0 for a group without members)
// and parts[g] = inv * risk_g, which ordered_sum adds to the loss.  Reads logp / target / weight below B * U, cost below B = G * N.
__global__ __launch_bounds__(256) void risk_weight_kernel(const float* __restrict__ logp, const int* __restrict__ target,
                                                          const float* __restrict__ weight, const float* __restrict__ cost, int G, int N,
                                                          int U, int V, double alpha, double inv, float* __restrict__ coef,
                                                          double* __restrict__ q_out, double* __restrict__ risk_out,
                                                          double* __restrict__ parts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long g = blockIdx.x * 4LL + wave; g < G; g += 4LL * gridDim.x) {
        const long long b = g * N + lane;
        const float cst = lane < N ? cost[b] : -1.0f;
        const bool member = cst >= 0.0f;
        double s = 0.0;
        if (member)
            for (int u = 0; u < U; ++u) {
                const int tg = target[b * U + u];
                const float wgt = weight[b * U + u];
                if (tg >= 0 && tg < V && wgt != 0.0f) s += (double)(wgt * logp[b * U + u]);
            }
        const double z = alpha * s;
        const unsigned long long members = __ballot(member);
        double M = -INFINITY;
        for (int i = 0; i < N; ++i) {
            const double zi = readlane_d(z, i);
            if ((members >> i) & 1ull) M = zi > M ? zi : M;               // (a NaN is passed by here and reaches Z through its own e)
        }
        const double e = member ? exp(z - M) : 0.0;
        double Z = 0.0;
        for (int i = 0; i < N; ++i) Z += readlane_d(e, i);
        const double q = member ? e / Z : 0.0;
        const double term = member ? q * (double)cst : 0.0;
        double risk = 0.0;
        for (int i = 0; i < N; ++i) risk += readlane_d(term, i);
        const double c = member ? alpha * q * ((double)cst - risk) * inv : 0.0;
        if (lane < N) { coef[b] = (float)c; q_out[b] = q; }
        if (lane == 0) { risk_out[g] = members ? risk : 0.0; parts[g] = members ? inv * risk : 0.0; }
    }
}
// One wave per logits row r = u * B + b, m and sum formed as softmax_ce_kernel forms them: dlogit[v] = coef[b] * w * ([v == t] - p_v),
// a zero row where the position is not scored (t outside [0, V), w = 0).  One store per element, by the lane that owns it; no LDS,
// no atomics.  Columns [V, Vp) are never read and written as zeros.
__global__ __launch_bounds__(256) void risk_grad_kernel(float* __restrict__ logits, const int* __restrict__ target,
                                                        const float* __restrict__ weight, const float* __restrict__ coef, long long rows,
                                                        int B, int U, int V, int Vp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long r = blockIdx.x * 4LL + wave; r < rows; r += 4LL * gridDim.x) {
        float* x = logits + r * Vp;
        const long long b = r % B, src = b * U + r / B;
        const int tg = target[src];
        const float wgt = weight[src];
        if (tg < 0 || tg >= V || wgt == 0.0f) {             // (the same in every lane)
            for (int v = lane; v < Vp; v += 64) x[v] = 0.0f;
            continue;
        }
        float m = -INFINITY;
        for (int v = lane; v < V; v += 64) m = fmaxf(m, x[v]);
        m = wave_butterfly(m, [](float a, float b) { return fmaxf(a, b); });
        float sum = 0.f;
        for (int v = lane; v < V; v += 64) sum += expf(x[v] - m);
        sum = wsum(sum);
        const float sc = coef[b] * wgt;
        for (int v = lane; v < Vp; v += 64) {
            float gvl = 0.f;
            if (v < V) gvl = sc * ((v == tg ? 1.0f : 0.0f) - expf(x[v] - m) / sum);
            x[v] = gvl;
        }
    }
}
void launch_risk_head(float* logits, const int* target, const float* weight, const float* cost, int B, int U, int V, int Vp, int N,
                      double alpha, double inv, float* logp, int* best, int* rank, float* coef, double* q, double* risk,
                      double* parts, double* loss, hipStream_t st) {
    const int G = B / N;
    const long long rows = (long long)B * U;
    const long long wgs = std::min<long long>((rows + 3) / 4, 2048);
    launch_score_rows(logits, target, B, U, V, Vp, logp, best, rank, st);
    hipLaunchKernelGGL(risk_weight_kernel, dim3((unsigned)std::min((G + 3) / 4, 2048)), dim3(256), 0, st, logp, target, weight, cost, G, N,
                       U, V, alpha, inv, coef, q, risk, parts);
    ordered_sum(parts, G, loss, st);
    hipLaunchKernelGGL(risk_grad_kernel, dim3((unsigned)wgs), dim3(256), 0, st, logits, target, weight, coef, rows, B, U, V, Vp);
}

// ---- the K likeliest entries and the entropy of every row (casv_score_get_alternatives) ----
// The order (alt_key) and the wave-wide maximum of its keys: alt_order.h, shared with the sampling pick (sample_kernels.hip).
// One wave per row, as score_rows_kernel, and its m, sum and validity formed by the same two loops (lane-strided, then the wave
// butterfly): logp has the bits of the head's logp for that index as target.  The row is read from memory once, into the wave's
// own Vp floats of LDS (no other wave touches them: no barrier); every later pass reads the entries the lane itself wrote.
// Selection: K rounds of a wave-wide maximum over the keys strictly below the previous winner's -- V/64 compares per lane and
// round, no scratch, no atomics, the same result whatever the launch shape.  Lane j keeps place j; the K places go out in one store.
__global__ __launch_bounds__(256) void score_alternatives_kernel(const float* __restrict__ logits, long long rows, int B, int U, int V,
                                                                 int Vp, int K, int* __restrict__ alt_idx, float* __restrict__ alt_logp,
                                                                 float* __restrict__ entropy) {
    extern __shared__ float alt_rows[];             // [4][Vp]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* s = alt_rows + wave * Vp;
    for (long long r = blockIdx.x * 4LL + wave; r < rows; r += 4LL * gridDim.x) {
        const float* x = logits + r * Vp;
        float m = -INFINITY;
        int nan = 0;
        for (int v = lane; v < V; v += 64) { const float xv = x[v]; s[v] = xv; nan |= xv != xv; m = fmaxf(m, xv); }
        m = wave_butterfly(m, [](float a, float b) { return fmaxf(a, b); });
        nan = wave_butterfly(nan, [](int a, int b) { return a | b; });
        const bool valid = !nan && m > -INFINITY && m < INFINITY;        // (the same in every lane)
        const long long src = (r % B) * U + r / B;
        int place = -1;
        float lp = __builtin_nanf(""), h = __builtin_nanf("");
        if (valid) {
            float sum = 0.f, dot = 0.f;
            for (int v = lane; v < V; v += 64) {
                const float xv = s[v], d = xv - m, e = expf(d);
                sum += e;
                if (xv > -INFINITY) dot += e * d;                        // (an -inf entry adds 0, not 0 * inf)
            }
            sum = wsum(sum);
            dot = wsum(dot);
            const float ls = logf(sum);
            h = ls - dot / sum;
            unsigned long long prev = ~0ull;
            for (int j = 0; j < K; ++j) {
                unsigned long long top = 0ull;
                for (int v = lane; v < V; v += 64) {
                    const unsigned long long key = alt_key(s[v], v);
                    if (key < prev && key > top) top = key;
                }
                top = wave_max_key(top);
                const int idx = (int)(0xffffffffu - (unsigned)top);      // (K <= V: every round finds one)
                const int own = (idx & ~63) | lane;                      // the winner's pass: its lane reads it, the wave gets it
                const float xw = __shfl(own < V ? s[own] : 0.f, idx & 63, 64);
                if (lane == j) { place = idx; lp = (xw - m) - ls; }
                prev = top;
            }
        }
        if (lane < K) { alt_idx[src * K + lane] = place; alt_logp[src * K + lane] = lp; }
        if (lane == 0 && entropy) entropy[src] = h;
    }
}
void launch_score_alternatives(const float* logits, int B, int U, int V, int Vp, int K, int* alt_idx, float* alt_logp, float* entropy,
                               hipStream_t st) {
    const long long rows = (long long)B * U;
    const long long wgs = std::min<long long>((rows + 3) / 4, 2048);
    hipLaunchKernelGGL(score_alternatives_kernel, dim3((unsigned)wgs), dim3(256), (size_t)4 * Vp * sizeof(float), st, logits, rows, B, U,
                       V, Vp, K, alt_idx, alt_logp, entropy);
}

// ... and the lines' sums: nll[b] = sum over the scored positions of -(double)logp[b][u], one thread per line adding in the order
// of u (one accumulator, no atomics: the same bits whatever the launch shape); count[b] = scored positions.
__global__ __launch_bounds__(64) void score_lines_kernel(const float* __restrict__ logp, const int* __restrict__ target, int B, int U,
                                                         int V, double* __restrict__ nll, int* __restrict__ count) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double acc = 0.0;
    int n = 0;
    for (int u = 0; u < U; ++u) {
        const int tg = target[(long long)b * U + u];
        if (tg < 0 || tg >= V) continue;
        acc += -(double)logp[(long long)b * U + u];
        ++n;
    }
    nll[b] = acc;
    count[b] = n;
}
void launch_score_lines(const float* logp, const int* target, int B, int U, int V, double* nll, int* count, hipStream_t st) {
    hipLaunchKernelGGL(score_lines_kernel, dim3((B + 63) / 64), dim3(64), 0, st, logp, target, B, U, V, nll, count);
}

// ... and the window form of the cell's attention rows in the caller's (B,U) order: lo = first position of step u's window (-1: the
// row is all NaN), w = its K weights (zeros beyond the window).  Ast [U+1][B][T] (row u + 1 belongs to step u), WIN [U][B].
__global__ __launch_bounds__(256) void score_extract_sparse_kernel(const float* __restrict__ Ast, const int* __restrict__ WIN, int B, int U,
                                                                   int T, int K, int* __restrict__ lo_out, float* __restrict__ w_out) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;       // (b, u)
    if (i >= (long long)B * U) return;
    const int b = (int)(i / U), u = (int)(i % U);
    const int win = WIN[(long long)u * B + b];
    const int lo = win & 0xffff, cnt = win >> 16;
    float* w = w_out + i * K;
    if (cnt <= 0) {
        lo_out[i] = -1;
        for (int k = 0; k < K; ++k) w[k] = __builtin_nanf("");
        return;
    }
    lo_out[i] = lo;
    const float* a = Ast + ((long long)(u + 1) * B + b) * T;
    for (int k = 0; k < K; ++k) w[k] = (k < cnt && lo + k < T) ? a[lo + k] : 0.0f;
}
void launch_score_extract_sparse(const float* Ast, const int* WIN, int B, int U, int T, int K, int* lo, float* w, hipStream_t st) {
    const long long n = (long long)B * U;
    hipLaunchKernelGGL(score_extract_sparse_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Ast, WIN, B, U, T, K, lo, w);
}

// ---- LSTM cell backward, pointwise part ----
// dh = a*mask_a + b + c ; gates/dz in the interleaved column order of the fused weight
__global__ void lstm_bwd_kernel(const LstmBwdBatch batch) {
    const LstmBwdArgs& p = batch.a[blockIdx.y];
    const int W = p.W;
    const long long n = (long long)p.rows * W;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / W; const int u = (int)(i % W);
        float dh = 0.f;
        if (p.a) dh += p.a[r * p.lda + u] * (p.mask_a ? p.mask_a[u] : 1.0f);
        if (p.b) dh += p.b[r * p.ldb + u];
        if (p.c) dh += p.c[r * p.ldc + u];
        const long long gi = r * 4 * W + (u >> 5) * 128 + (u & 31);
        const float ig = p.gates[gi], fg = p.gates[gi + 32], gg = p.gates[gi + 64], og = p.gates[gi + 96];
        const float cc = p.cell[r * W + u];
        const float cp = p.c_prev ? p.c_prev[r * p.ld_cprev + u] : 0.0f;
        const LstmCellBwdOut d = lstm_cell_bwd(dh, ig, fg, gg, og, cc, cp, p.dc[r * W + u]);
        p.dz[gi] = d.zi;
        p.dz[gi + 32] = d.zf;
        p.dz[gi + 64] = d.zg;
        p.dz[gi + 96] = d.zo;
        p.dc[r * W + u] = d.dc;
    }
}
void launch_lstm_bwd_batch(const LstmBwdBatch& b, hipStream_t st) {
    if (b.count < 1) return;
    long long n = 0;
    for (int j = 0; j < b.count; ++j) n = std::max(n, (long long)b.a[j].rows * b.a[j].W);
    hipLaunchKernelGGL(lstm_bwd_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 4096), b.count), dim3(256), 0, st, b);
}
void launch_lstm_bwd(const LstmBwdArgs& p, hipStream_t st) {
    LstmBwdBatch b{};
    b.a[0] = p; b.count = 1;
    launch_lstm_bwd_batch(b, st);
}

// ---- attention backward for one decoder time step (oracle/train.py; no gradient through the window
// mask nor through the previous alignment, attention.py:567) ----
// One workgroup per sample.  Everything that is read is independent of what is written, so the loads batch; the
// read-modify-writes of d_enc / du go out as fire-and-forget float atomics (distinct addresses: no contention).
// dva / dbv are kept as per-sample partial sums across the steps and reduced once after the loop.
template <bool ORDERED>
__global__ __launch_bounds__(256) void attention_bwd_kernel(const AttnBwdArgs p) {
    __shared__ float s_dx[2048];
    __shared__ float s_da[16], s_ds[16], s_av[16];
    attention_bwd_sample<false, 0, ORDERED>(p, blockIdx.x, true, threadIdx.x, 256, s_dx, s_da, s_ds, s_av);
}
// ---- the deferred sums of the attention backward (attn_bwd.h, DEFER): one wave per (sample, 64 columns), its share of the
// sample's [T][64] sums in LDS, one pass over the steps (loads of four steps in flight together) ----
__global__ __launch_bounds__(64) void attention_deferred_enc_kernel(const AttnDeferArgs p) {
    extern __shared__ float s_acc[];                          // [T][64]
    const int lane = threadIdx.x, c = blockIdx.x * 64 + lane, b = blockIdx.y;
    const int T = p.T, B = p.B;
    for (int s = 0; s < T; ++s) s_acc[s * 64 + lane] = 0.0f;
    const float mk = p.mcell ? p.mcell[(long long)b * p.ld_mcell + p.mc_off + c] : 1.0f;
    constexpr int NB = 4;
    for (int t0 = 0; t0 < p.U; t0 += NB) {
        float dx[NB], av[NB]; int wv[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int t = t0 + j < p.U ? t0 + j : p.U - 1;
            wv[j] = p.WIN[(long long)t * B + b];
            dx[j] = p.dRec[((long long)t * B + b) * p.ld_drec + c];
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int t = t0 + j < p.U ? t0 + j : p.U - 1;
            const int s_lo = wv[j] & 0xffff, cnt = wv[j] >> 16;
            av[j] = lane < cnt ? p.Ast[((long long)(t + 1) * B + b) * T + s_lo + lane] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if (t0 + j < p.U) {
                const int s_lo = wv[j] & 0xffff, cnt = wv[j] >> 16;
                const float d = dx[j] * mk;
                for (int i = 0; i < cnt; ++i) s_acc[(s_lo + i) * 64 + lane] += __shfl(av[j], i, 64) * d;
            }
        }
    }
    for (int s = 0; s < T; ++s) {
        float* o = p.d_enc + ((long long)s * B + b) * p.C + c;
        *o += s_acc[s * 64 + lane];
    }
}
__global__ __launch_bounds__(64) void attention_deferred_u_kernel(const AttnDeferArgs p) {
    extern __shared__ float s_acc[];                          // [T][64]
    const int lane = threadIdx.x, j = blockIdx.x * 64 + lane, b = blockIdx.y;
    const int T = p.T, B = p.B, W = p.W;
    for (int s = 0; s < T; ++s) s_acc[s * 64 + lane] = 0.0f;
    const float v = p.va[j];
    const float* ub = p.u + (long long)b * W + j;             // u[s][b][j] = ub[s * B * W]
    for (int t = 0; t < p.U; ++t) {
        const int wv = p.WIN[(long long)t * B + b];
        const float q = p.WQ[((long long)t * B + b) * W + j];
        const float ds = lane < 16 ? p.DS[((long long)t * B + b) * 16 + lane] : 0.0f;
        const int s_lo = wv & 0xffff, cnt = wv >> 16;
        float uu[11];
#pragma unroll
        for (int i = 0; i < 11; ++i) uu[i] = ub[(long long)(s_lo + (i < cnt ? i : 0)) * B * W];
#pragma unroll
        for (int i = 0; i < 11; ++i) {
            const float th = fast_tanh(q + uu[i]);
            const float dpre = __shfl(ds, i, 64) * v * (1.0f - th * th);
            if (i < cnt) s_acc[(s_lo + i) * 64 + lane] += dpre;
        }
    }
    for (int s = 0; s < T; ++s) {
        float* o = p.du + ((long long)s * B + b) * W + j;
        *o += s_acc[s * 64 + lane];
    }
}
void launch_attention_deferred(const AttnDeferArgs& p, hipStream_t st) {
    static bool attr_set[64] = {false};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_deferred_enc_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, ATTN_DEFER_MAX_T * 64 * 4);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_deferred_u_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, ATTN_DEFER_MAX_T * 64 * 4);
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    if (p.what & 1) hipLaunchKernelGGL(attention_deferred_enc_kernel, dim3(p.C / 64, p.B), dim3(64), (size_t)p.T * 64 * 4, st, p);
    if (p.what & 2) hipLaunchKernelGGL(attention_deferred_u_kernel, dim3(p.W / 64, p.B), dim3(64), (size_t)p.T * 64 * 4, st, p);
}

void launch_attention_bwd(const AttnBwdArgs& p, hipStream_t st, bool ordered) {
    if (ordered) hipLaunchKernelGGL(attention_bwd_kernel<true>, dim3(p.B), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(attention_bwd_kernel<false>, dim3(p.B), dim3(256), 0, st, p);
}

__global__ void axpy_kernel(float* __restrict__ y, const float* __restrict__ x, long long n) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) y[i] += x[i];
}
void launch_axpy(float* y, const float* x, long long n, hipStream_t st) {
    hipLaunchKernelGGL(axpy_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 2048)), dim3(256), 0, st, y, x, n);
}

// ---- out[c] += sum_r in[r][c] ----
__global__ void colsum_kernel(const float* __restrict__ in, long long rows, int cols, long long ld, float* __restrict__ out,
                              int rows_per_block) {
    __shared__ float part[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.y * rows_per_block;
    const long long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    float s = 0.f;
    if (c < cols)
        for (long long r = r0 + rl; r < r1; r += 4) s += in[r * ld + c];
    part[rl][threadIdx.x & 63] = s;
    __syncthreads();
    if (rl == 0 && c < cols) atomicAdd(out + c, part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}
// ... one thread per column, the rows in order
__global__ void colsum_ordered_kernel(const float* __restrict__ in, long long rows, int cols, long long ld, float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
    for (long long r = 0; r < rows; ++r) s += in[r * ld + c];
    out[c] += s;
}
void launch_colsum(const float* in, long long rows, int cols, long long ld, float* out, hipStream_t st, bool ordered) {
    if (ordered) { hipLaunchKernelGGL(colsum_ordered_kernel, dim3((cols + 255) / 256), dim3(256), 0, st, in, rows, cols, ld, out); return; }
    const int rpb = 512;
    hipLaunchKernelGGL(colsum_kernel, dim3((cols + 63) / 64, (unsigned)((rows + rpb - 1) / rpb)), dim3(256), 0, st, in, rows, cols, ld, out, rpb);
}

// ---- embedding regulariser (seq2seq.py:530-553): value and gradient ----
//   1 * sum_w (E[0][w] - stopgrad(mean_{v>=1} E[v][w]))^2  +  0.01 * sum_v (1 - |E[v]|^2)^2
// Two small grids instead of one workgroup walking the whole table (0.54 ms of the step): columns in blocks of 64 (four row
// groups per block meet in LDS), rows one wave each.  The gradient is added in place: every contribution to dE of this step
// has been queued on the same stream before.
template <bool ORDERED>        // ORDERED: loss = parts, one value per workgroup (cols) / row (rows), added by ordered_sum
__global__ __launch_bounds__(256) void reg_cols_kernel(const float* __restrict__ E, float* __restrict__ dE, int V, int W,
                                                       double* __restrict__ loss, int want_grad) {
    __shared__ float part[4][64];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6, w = blockIdx.x * 64 + c;
    float s = 0.f;
    if (w < W) for (int v = 1 + g; v < V; v += 4) s += E[(long long)v * W + w];
    part[g][c] = s;
    __syncthreads();
    float sq = 0.f;
    if (g == 0 && w < W) {
        const float mr = (part[0][c] + part[1][c] + part[2][c] + part[3][c]) / (float)(V - 1);
        const float d = E[w] - mr;
        sq = d * d;
        if (want_grad) dE[w] += 2.0f * d;
    }
    if (g == 0) {
        sq = wsum(sq);
        if (c == 0) { if (ORDERED) loss[blockIdx.x] = (double)sq; else atomicAdd(loss, (double)sq); }
    }
}
template <bool ORDERED>
__global__ __launch_bounds__(256) void reg_rows_kernel(const float* __restrict__ E, float* __restrict__ dE, int V, int W,
                                                       double* __restrict__ loss, int want_grad) {
    const int lane = threadIdx.x & 63, v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= V) return;
    const float* row = E + (long long)v * W;
    float n = 0.f;
    for (int w = lane; w < W; w += 64) n += row[w] * row[w];
    n = wsum(n);
    if (want_grad) {
        const float k = -0.04f * (1.0f - n);
        for (int w = lane; w < W; w += 64) dE[(long long)v * W + w] += k * row[w];
    }
    if (lane == 0) {
        if (ORDERED) loss[v] = (double)(0.01f * (1.0f - n) * (1.0f - n));
        else atomicAdd(loss, (double)(0.01f * (1.0f - n) * (1.0f - n)));
    }
}
void launch_reg(const float* E, float* dE, int V, int W, double* loss, int want_grad, hipStream_t st, double* parts) {
    if (parts) {            // parts [(W + 63) / 64 + V]
        const int nc = (W + 63) / 64;
        hipLaunchKernelGGL(reg_cols_kernel<true>, dim3(nc), dim3(256), 0, st, E, dE, V, W, parts, want_grad);
        hipLaunchKernelGGL(reg_rows_kernel<true>, dim3((V + 3) / 4), dim3(256), 0, st, E, dE, V, W, parts + nc, want_grad);
        ordered_sum(parts, nc + V, loss, st);
        return;
    }
    hipLaunchKernelGGL(reg_cols_kernel<false>, dim3((W + 63) / 64), dim3(256), 0, st, E, dE, V, W, loss, want_grad);
    hipLaunchKernelGGL(reg_rows_kernel<false>, dim3((V + 3) / 4), dim3(256), 0, st, E, dE, V, W, loss, want_grad);
}

// ---- global gradient norm and Adam (Keras Adam(clipnorm)) ----
__global__ void sumsq_kernel(const float* __restrict__ g, long long n, double* __restrict__ acc) {
    __shared__ double red[256];
    double s = 0.0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const double v = g[i]; s += v * v;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) atomicAdd(acc, red[0]);
}
void launch_sumsq(const float* g, long long n, double* acc, hipStream_t st) {
    hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 1024)), dim3(256), 0, st, g, n, acc);
}

__global__ void adam_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            long long n, const double* __restrict__ normsq, float clipnorm, float lr_t, float b1, float b2, float eps) {
    const float norm = (float)sqrt(*normsq);
    const float scale = (clipnorm > 0.f && norm >= clipnorm) ? clipnorm / norm : 1.0f;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float gi = g[i] * scale;
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        w[i] -= lr_t * mi / (sqrtf(vi) + eps);
    }
}
void launch_adam(float* w, const float* g, float* m, float* v, long long n, const double* normsq, float clipnorm, float lr_t,
                 float b1, float b2, float eps, hipStream_t st) {
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 2048)), dim3(256), 0, st, w, g, m, v, n,
                       normsq, clipnorm, lr_t, b1, b2, eps);
}

// ---- the same over a list of tensors, one launch each ----
bool multi_add(MultiTensor& mt, float* w, float* g, float* m, float* v, long long n, int max_blocks) {
    if (mt.count >= MULTI_MAX || n < 1) return n < 1;
    const int k = mt.count++;
    mt.w[k] = w; mt.g[k] = g; mt.m[k] = m; mt.v[k] = v; mt.n[k] = n;
    if (k == 0) mt.first_block[0] = 0;
    mt.first_block[k + 1] = mt.first_block[k] + (int)std::min<long long>((n + 255) / 256, max_blocks);
    return true;
}
__device__ __forceinline__ int multi_find(const MultiTensor& mt, const int block) {      // (uniform per workgroup: scalar code)
    int k = 0;
    while (k + 1 < mt.count && block >= mt.first_block[k + 1]) ++k;
    return k;
}
template <bool ORDERED>        // ORDERED: acc = parts, one value per workgroup (added by ordered_sum)
__global__ void sumsq_multi_kernel(const MultiTensor mt, double* __restrict__ acc) {
    __shared__ double red[256];
    const int k = multi_find(mt, blockIdx.x);
    const float* __restrict__ g = mt.g[k];
    const long long n = mt.n[k], stride = (long long)(mt.first_block[k + 1] - mt.first_block[k]) * blockDim.x;
    double s = 0.0;
    for (long long i = (long long)(blockIdx.x - mt.first_block[k]) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double v = g[i]; s += v * v;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) { if (ORDERED) acc[blockIdx.x] = red[0]; else atomicAdd(acc, red[0]); }
}
void launch_sumsq_multi(const MultiTensor& mt, double* acc, hipStream_t st, double* parts) {
    if (mt.count < 1) return;
    if (parts) {            // parts [first_block[count]] (<= MULTI_MAX * the caller's max_blocks)
        hipLaunchKernelGGL(sumsq_multi_kernel<true>, dim3((unsigned)mt.first_block[mt.count]), dim3(256), 0, st, mt, parts);
        ordered_sum(parts, mt.first_block[mt.count], acc, st);
        return;
    }
    hipLaunchKernelGGL(sumsq_multi_kernel<false>, dim3((unsigned)mt.first_block[mt.count]), dim3(256), 0, st, mt, acc);
}
__global__ void adam_multi_kernel(const MultiTensor mt, const double* __restrict__ normsq, float clipnorm, float lr_t, float b1, float b2,
                                  float eps) {
    const int k = multi_find(mt, blockIdx.x);
    float* __restrict__ w = mt.w[k]; const float* __restrict__ g = mt.g[k]; float* __restrict__ m = mt.m[k]; float* __restrict__ v = mt.v[k];
    const long long n = mt.n[k], stride = (long long)(mt.first_block[k + 1] - mt.first_block[k]) * blockDim.x;
    const float norm = (float)sqrt(*normsq);
    const float scale = (clipnorm > 0.f && norm >= clipnorm) ? clipnorm / norm : 1.0f;
    for (long long i = (long long)(blockIdx.x - mt.first_block[k]) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float gi = g[i] * scale;
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        w[i] -= lr_t * mi / (sqrtf(vi) + eps);
    }
}
void launch_adam_multi(const MultiTensor& mt, const double* normsq, float clipnorm, float lr_t, float b1, float b2, float eps, hipStream_t st) {
    if (mt.count < 1) return;
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)mt.first_block[mt.count]), dim3(256), 0, st, mt, normsq, clipnorm, lr_t, b1, b2, eps);
}

}  // namespace casv
