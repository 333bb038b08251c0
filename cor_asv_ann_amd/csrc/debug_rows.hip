// Test support: one row head alone on the caller's logits -- the scoring head and the alternatives (score.hip's), the sampling picks
// (decode.hip's), the soft and the risk loss heads (train.hip's), the scheduled-sampling mix (train_sched.hip's).  Every entry lays
// the caller's rows out as the library does (StagedRows), holds its device operands in a DebugBuffers, launches the head once and
// copies the results back.  A fresh output buffer holds 0xFF bytes; what a head adds into is cleared.
#include "train_step.h"

namespace {

int check_rows(int R, int V) { return R < 1 || R > (1 << 20) || V < 1 || V > 4096 ? fail(CASV_ERR_ARG, "R must be in [1, 2^20], V in [1, 4096]") : CASV_OK; }

// The caller's logits (B,U,V) as the step lays them out: row u * B + b, the library's row stride Vp (engine.hip, casv_model_create),
// the padding columns filled with pad_value.  R rows without steps are B = R, U = 1: row r.
struct StagedRows {
    int B, U, V, Vp;
    std::vector<float> x;
    StagedRows(const float* logits, int B_, int U_, int V_, float pad_value)
        : B(B_), U(U_), V(V_), Vp((V_ + 31) & ~31), x((size_t)B_ * U_ * Vp, pad_value) {
        for (int b = 0; b < B; ++b)
            for (int u = 0; u < U; ++u) memcpy(row(b, u), logits + ((size_t)b * U + u) * V, (size_t)V * 4);
    }
    float* row(int b, int u) { return &x[((size_t)u * B + b) * Vp]; }
    float* upload(DebugBuffers& bufs, int& rc) { return static_cast<float*>(bufs.put(x.data(), x.size(), rc)); }
    // Waits for the stream; with `out`, brings the device rows back first and hands the caller their V columns, once a head that
    // wrote gradients into them has left zeros in the padding (`head`: its name; by_step: the message names (b, u), not the row).
    int fetch(hipStream_t st, const float* dev, float* out, const char* head, bool by_step) {
        if (out) HIPCHK(hipMemcpyAsync(x.data(), dev, x.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int b = 0; b < B && out; ++b)
            for (int u = 0; u < U; ++u) {
                const float* r = row(b, u);
                for (int v = V; v < Vp; ++v) {
                    if (r[v] == 0.f) continue;
                    if (by_step) return fail(CASV_ERR_HIP, "%s: padding column %d of row (%d, %d) is %g, not zero", head, v, b, u, (double)r[v]);
                    return fail(CASV_ERR_HIP, "%s: padding column %d of row %d is %g, not zero", head, v, b, (double)r[v]);
                }
                memcpy(out + ((size_t)b * U + u) * V, r, (size_t)V * 4);
            }
        return CASV_OK;
    }
};

// put() with the element type: n elements of T (4 or 8 bytes each) copied from src, or (nullptr) 0xFF bytes
template <class T> T* put(DebugBuffers& bufs, const T* src, size_t n, int& rc) {
    static_assert(sizeof(T) % 4 == 0, "DebugBuffers::put counts 4-byte elements");
    return rc ? nullptr : static_cast<T*>(bufs.put(src, n * (sizeof(T) / 4), rc));
}
const double kZeroLoss[2] = {0.0, 0.0};        // the 16 bytes a loss head adds its sums into

}  // namespace

// The scoring head (launch_score_rows).
extern "C" int casv_debug_score_rows(casv_model* m, int32_t R, int32_t V, const float* logits, const int32_t* target, float pad_value,
                                     float* logp, int32_t* best, int32_t* rank) {
    if (!m || !logits || !target || !logp || !best || !rank) return fail(CASV_ERR_ARG, "null argument");
    if (int rc = check_rows(R, V)) return rc;
    HIPCHK(hipSetDevice(m->device));
    StagedRows rows(logits, R, 1, V, pad_value);
    DebugBuffers bufs{m->stream};
    int rc = 0;
    const float* dx = rows.upload(bufs, rc);
    const int* dt = put(bufs, target, R, rc);
    float* dl = put<float>(bufs, nullptr, R, rc);
    int* db = put<int>(bufs, nullptr, R, rc);
    int* dr = put<int>(bufs, nullptr, R, rc);
    if (rc) return rc;
    launch_score_rows(dx, dt, R, 1, V, rows.Vp, dl, db, dr, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(logp, dl, (size_t)R * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(best, db, (size_t)R * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(rank, dr, (size_t)R * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}

// score_alternatives_kernel.
extern "C" int casv_debug_alternatives_rows(casv_model* m, int32_t R, int32_t V, int32_t K, const float* logits, float pad_value,
                                            int32_t* alt_idx, float* alt_logp, float* entropy) {
    if (!m || !logits || !alt_idx || !alt_logp) return fail(CASV_ERR_ARG, "null argument");
    if (int rc = check_rows(R, V)) return rc;
    if (K < 1 || K > V || K > 64) return fail(CASV_ERR_ARG, "K=%d outside [1, min(V, 64)] = [1, %d]", K, V < 64 ? V : 64);
    HIPCHK(hipSetDevice(m->device));
    StagedRows rows(logits, R, 1, V, pad_value);
    DebugBuffers bufs{m->stream};
    int rc = 0;
    const float* dx = rows.upload(bufs, rc);
    int* di = put<int>(bufs, nullptr, (size_t)R * K, rc);
    float* dl = put<float>(bufs, nullptr, (size_t)R * K, rc);
    float* de = put<float>(bufs, nullptr, R, rc);
    if (rc) return rc;
    launch_score_alternatives(dx, R, 1, V, rows.Vp, K, di, dl, entropy ? de : nullptr, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(alt_idx, di, (size_t)R * K * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(alt_logp, dl, (size_t)R * K * 4, hipMemcpyDeviceToHost, m->stream));
    if (entropy) HIPCHK(hipMemcpyAsync(entropy, de, (size_t)R * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}

// sample_kernel (cut == nullptr) or sample_cut_kernel.
static int debug_sample_rows(casv_model* m, int32_t R, int32_t V, const casv_sample_params* p, const casv_sample_cut* cut, int32_t step,
                             const int64_t* stream, const int32_t* sample, const float* logits, const float* u, float pad_value, int32_t* out_idx,
                             float* out_logp, float* out_logq, float* out_feedback) {
    if (!logits || !out_feedback) return fail(CASV_ERR_ARG, "null argument");
    if (!m || !p || !out_idx || !out_logp || !out_logq) return fail(CASV_ERR_ARG, "null argument");
    if (!(p->temperature > 0.f) || !(p->temperature < INFINITY)) return fail(CASV_ERR_ARG, "temperature=%g must be finite and positive", (double)p->temperature);
    if (p->top_k < 0 || p->top_k > 64) return fail(CASV_ERR_ARG, "top_k=%d out of range 0..64", p->top_k);
    if (int rc = check_rows(R, V)) return rc;
    if (step < 0 || step >= 2 * CASV_MAX_T) return fail(CASV_ERR_ARG, "step=%d out of range 0..%d", step, 2 * CASV_MAX_T - 1);
    HIPCHK(hipSetDevice(m->device));
    if (cut && !sample_cut_ready()) return fail(CASV_ERR_HIP, "the runtime refused sample_cut_kernel's %d bytes of dynamic LDS", SAMPLE_CUT_LDS);
    StagedRows rows(logits, R, 1, V, pad_value);
    const int Vp = rows.Vp;
    DebugBuffers bufs{m->stream};
    int rc = 0;
    SampleArgs a{};
    a.logits = rows.upload(bufs, rc);
    // (the output slot is step + 1 of a store whose slots all lie on the one (R,Vp) buffer)
    a.feedback = put<float>(bufs, nullptr, (size_t)R * Vp, rc);
    a.fb_slot = 0; a.R = R; a.V = V; a.step_imm = step; a.rows_per_line = 1;
    if (stream) a.stream = put(bufs, reinterpret_cast<const long long*>(stream), R, rc);
    if (sample) a.sample = put(bufs, sample, R, rc);
    if (u) a.u = put(bufs, u, R, rc);
    a.seed = p->seed; a.temperature = p->temperature; a.top_k = p->top_k;
    a.out_idx = put<int>(bufs, nullptr, R, rc);
    a.out_logp = put<float>(bufs, nullptr, R, rc);
    a.out_logq = put<float>(bufs, nullptr, R, rc);
    if (rc) return rc;
    a.S = 1; a.out_col = 0;
    hipEvent_t ev{};
    m->prof_begin(PC_SAMPLE, 4.0 * R * V, 4.0 * R * (V + Vp), ev);
    if (cut) {
        a.top_k = cut->top_k; a.top_p = cut->top_p;
        m->stat_sample_cut_rows = launch_sample_cut(a, m->sample_cut_rows_opt, m->stream);
    } else launch_sample(a, m->stream);
    m->prof_end(PC_SAMPLE, ev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_idx, a.out_idx, (size_t)R * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_logp, a.out_logp, (size_t)R * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_logq, a.out_logq, (size_t)R * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_feedback, a.feedback, (size_t)R * Vp * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->prof.on) m->prof.collect();
    return CASV_OK;
}

extern "C" int casv_debug_sample_rows(casv_model* m, int32_t R, int32_t V, const casv_sample_params* p, int32_t step, const int64_t* stream,
                                      const int32_t* sample, const float* logits, const float* u, float pad_value, int32_t* out_idx,
                                      float* out_logp, float* out_logq, float* out_feedback) {
    return debug_sample_rows(m, R, V, p, nullptr, step, stream, sample, logits, u, pad_value, out_idx, out_logp, out_logq, out_feedback);
}

extern "C" int casv_debug_sample_cut_rows(casv_model* m, int32_t R, int32_t V, const casv_sample_params* p, const casv_sample_cut* cut,
                                          int32_t step, const int64_t* stream, const int32_t* sample, const float* logits, const float* u,
                                          float pad_value, int32_t* out_idx, float* out_logp, float* out_logq, float* out_feedback) {
    if (int rc = check_sample_cut(cut)) return rc;
    if (p && p->top_k != 0) return fail(CASV_ERR_ARG, "top_k=%d beside a cut: the cut carries it", p->top_k);
    return debug_sample_rows(m, R, V, p, cut, step, stream, sample, logits, u, pad_value, out_idx, out_logp, out_logq, out_feedback);
}

// soft_ce_kernel (B = R, U = 1).
extern "C" int casv_debug_soft_ce_rows(casv_model* m, int32_t R, int32_t V, int32_t K, const float* logits, const int32_t* soft_idx,
                                       const float* soft_q, const float* weight, float inv_count, float pad_value, int32_t want_grad,
                                       double* loss, float* dlogits, int32_t ordered) {
    if (!m || !logits || !soft_idx || !soft_q || !weight || !loss || (want_grad && !dlogits)) return fail(CASV_ERR_ARG, "null argument");
    if (int rc = check_rows(R, V)) return rc;
    if (int rc = check_soft_targets(R, K, V, soft_idx, soft_q)) return rc;
    HIPCHK(hipSetDevice(m->device));
    StagedRows rows(logits, R, 1, V, pad_value);
    DebugBuffers bufs{m->stream};
    int rc = 0;
    float* dx = rows.upload(bufs, rc);
    const int* di = put(bufs, soft_idx, (size_t)R * K, rc);
    const float* dq = put(bufs, soft_q, (size_t)R * K, rc);
    const float* dw = put(bufs, weight, R, rc);
    double* dl = put(bufs, kZeroLoss, 2, rc);
    double* dp = put<double>(bufs, nullptr, 2048, rc);          // (launch_soft_ce: at most 2048 workgroups, each writes its part)
    if (rc) return rc;
    launch_soft_ce(dx, di, dq, dw, R, 1, V, rows.Vp, K, inv_count, dl, want_grad ? 1 : 0, m->stream, ordered ? dp : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(loss, dl, 8, hipMemcpyDeviceToHost, m->stream));
    return rows.fetch(m->stream, dx, want_grad ? dlogits : nullptr, "soft head", false);
}

// The risk head on logits (B = G * N, U, V) in the caller's (b, u) order -- casv_debug_soft_ce_rows with U steps.
extern "C" int casv_debug_risk_rows(casv_model* m, int32_t G, int32_t N, int32_t U, int32_t V, const float* logits, const int32_t* target,
                                    const float* weight, const float* cost, double alpha, float pad_value, int32_t want_grad,
                                    double* loss, double* q, float* coef, float* dlogits) {
    if (!m || !logits || !target || !weight || !loss || !q || !coef || (want_grad && !dlogits)) return fail(CASV_ERR_ARG, "null argument");
    if (G < 1 || U < 1 || V < 1 || V > 4096 || N < 1 || N > 64 || (long long)G * N * U > (1 << 20))
        return fail(CASV_ERR_ARG, "G, U >= 1, N in [1, 64], G * N * U <= 2^20, V in [1, 4096]");
    const int B = G * N;
    const size_t R = (size_t)B * U;
    double inv = 1.0;
    if (int rc = check_risk(B, N, cost, alpha, &inv)) return rc;
    for (size_t i = 0; i < R; ++i)
        if (target[i] < -1 || target[i] >= V) return fail(CASV_ERR_ARG, "target[%zu] = %d outside [-1, %d)", i, target[i], V);
    HIPCHK(hipSetDevice(m->device));
    StagedRows rows(logits, B, U, V, pad_value);
    DebugBuffers bufs{m->stream};
    int rc = 0;
    float* dx = rows.upload(bufs, rc);
    const int* dt = put(bufs, target, R, rc);
    const float* dw = put(bufs, weight, R, rc);
    const float* dc = put(bufs, cost, B, rc);
    double* dl = put(bufs, kZeroLoss, 2, rc);
    float* dlogp = put<float>(bufs, nullptr, R, rc);
    int* dbest = put<int>(bufs, nullptr, R, rc);
    int* drank = put<int>(bufs, nullptr, R, rc);
    float* dcoef = put<float>(bufs, nullptr, B, rc);
    double* dq = put<double>(bufs, nullptr, B, rc);
    double* drisk = put<double>(bufs, nullptr, G, rc);
    double* dparts = put<double>(bufs, nullptr, G, rc);         // (every group writes its part)
    if (rc) return rc;
    launch_risk_head(dx, dt, dw, dc, B, U, V, rows.Vp, N, alpha, inv, dlogp, dbest, drank, dcoef, dq, drisk, dparts, dl, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(loss, dl, 8, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(q, dq, (size_t)B * 8, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(coef, dcoef, (size_t)B * 4, hipMemcpyDeviceToHost, m->stream));
    return rows.fetch(m->stream, dx, want_grad ? dlogits : nullptr, "risk head", true);
}

// The mix kernel of scheduled sampling, under the cut if one is given.
static int debug_sched_rows(casv_model* m, int32_t R, int32_t V, const casv_sched_params* p, const casv_sample_cut* cut, const int32_t* b,
                            const int32_t* u, const float* logits, const int32_t* gold, float pad_value, int32_t* out) {
    if (!m || !b || !u || !logits || !gold || !out) return fail(CASV_ERR_ARG, "null argument");
    if (int rc = check_sched_params(p, false)) return rc;
    if (int rc = cut ? check_sched_cut(p, cut) : 0) return rc;
    if (int rc = check_rows(R, V)) return rc;
    HIPCHK(hipSetDevice(m->device));
    if (cut && !sched_mix_cut_ready()) return fail(CASV_ERR_HIP, "the runtime refused sched_mix_cut_kernel's %d bytes of dynamic LDS", SAMPLE_CUT_LDS);
    StagedRows rows(logits, R, 1, V, pad_value);
    DebugBuffers bufs{m->stream};
    int rc = 0;
    SchedMixArgs a{};
    a.logits = rows.upload(bufs, rc);
    a.gold = put(bufs, gold, R, rc);
    a.row_b = put(bufs, b, R, rc);
    a.row_u = put(bufs, u, R, rc);
    a.out = put<int>(bufs, nullptr, R, rc);
    if (rc) return rc;
    a.R = R; a.B = R; a.U = 1; a.V = V; a.Vp = rows.Vp;
    a.seed = p->seed; a.step_id = p->step_id; a.ratio = p->ratio; a.temperature = p->temperature; a.pick = p->pick;
    if (cut) { a.top_k = cut->top_k; a.top_p = cut->top_p; }
    launch_sched_mix(a, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, a.out, (size_t)R * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}

extern "C" int casv_debug_sched_rows(casv_model* m, int32_t R, int32_t V, const casv_sched_params* p, const int32_t* b, const int32_t* u,
                                     const float* logits, const int32_t* gold, float pad_value, int32_t* out) {
    return debug_sched_rows(m, R, V, p, nullptr, b, u, logits, gold, pad_value, out);
}

extern "C" int casv_debug_sched_cut_rows(casv_model* m, int32_t R, int32_t V, const casv_sched_params* p, const casv_sample_cut* cut,
                                         const int32_t* b, const int32_t* u, const float* logits, const int32_t* gold, float pad_value,
                                         int32_t* out) {
    if (!cut) return fail(CASV_ERR_ARG, "null argument");
    return debug_sched_rows(m, R, V, p, cut, b, u, logits, gold, pad_value, out);
}
