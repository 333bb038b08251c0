// Scoring: teacher-forced log-probabilities of given targets (kt:407 / s2s:491-497, the forward pass of a mode-0 step).
// casv_score_targets makes the same two attempts as casv_train_step (score_attempt): phases 1-4 of the step as they are (train_step.h),
// then the projection and the scoring head in place of the loss -- give-up check; on a forward-only state outside a session.
// casv_score_candidates is the same call with N targets per source: the encoder side of the forward phases works on the Be sources,
// the decoder side on the B = Be * N rows (Step::Be / N, TLayer::rows); casv_train_step and casv_score_targets have Be = B, N = 1.
#include "train_step.h"

// What a scoring call hands back: (B,U) arrays in the caller's order, (B) sums, the dense alignment rows (B,U,T) or nullptr.
struct ScoreOut { float* logp; int32_t* best; int32_t* rank; double* nll; int32_t* count; float* align; };

// The head: log-probability, argmax and rank of every row, the lines' sums; leaves them on the device in the caller's order.
static int score_head(Step& s) {
    TrainState* ts = s.ts; hipStream_t st = s.st;
    const int B = s.B, U = s.U, V = s.V, Vp = s.Vp;
    if (int rc = projection(s)) return rc;
    launch_score_rows(ts->logits.as<float>(), ts->d_out.as<int>(), B, U, V, Vp, ts->s_logp.as<float>(), ts->s_best.as<int>(),
                      ts->s_rank.as<int>(), st);
    launch_score_lines(ts->s_logp.as<float>(), ts->d_out.as<int>(), B, U, V, ts->s_nll.as<double>(), ts->s_count.as<int>(), st);
    return 0;
}

// One attempt at a scoring call: the first four phases of the step, the scoring head, the give-up check (as a mode-0 step:
// *redo -- a persistent forward recurrence gave up, the back-off is set and the caller starts over).
static int score_attempt(Step s, const ScoreOut& out, bool* redo) {
    casv_model* m = s.m; TrainState* ts = s.ts; hipStream_t st = s.st;
    const int B = s.B, T = s.T, U = s.U;
    ts->B = B; ts->Be = s.Be; ts->N = s.N; ts->T = T; ts->U = U; ts->A = s.A;
    ts->score_B = 0;
    m->encoded = false;                    // the final-state buffers are shared with the inference session
    if (int rc = plan_buffers(s)) return rc;
    if (int rc = ts->s_logp.ensure(s.UB * 4)) return rc;
    if (int rc = ts->s_best.ensure(s.UB * 4)) return rc;
    if (int rc = ts->s_rank.ensure(s.UB * 4)) return rc;
    if (int rc = ts->s_nll.ensure((size_t)B * 8)) return rc;
    if (int rc = ts->s_count.ensure((size_t)B * 4)) return rc;
    if (int rc = stage_inputs(s)) return rc;
    if (int rc = forward_layers(s)) return rc;
    if (int rc = forward_cell(s)) return rc;
    if (int rc = score_head(s)) return rc;
    HIPCHK(hipGetLastError());
    if (int rc = recurrences_gave_up(m, *redo)) return rc;
    if (*redo) return CASV_OK;
    HIPCHK(hipMemcpyAsync(out.logp, ts->s_logp.p, s.UB * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out.best, ts->s_best.p, s.UB * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out.rank, ts->s_rank.p, s.UB * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out.nll, ts->s_nll.p, (size_t)B * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out.count, ts->s_count.p, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    std::vector<float> rows;               // the attention rows as the cell left them, [U][B][T] behind the initial row
    if (out.align) {
        rows.resize((size_t)s.UB * T);
        HIPCHK(hipMemcpyAsync(rows.data(), ts->Ast.as<float>() + (size_t)B * T, rows.size() * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (int b = 0; b < B && out.align; ++b)
        for (int u = 0; u < U; ++u)
            memcpy(out.align + ((size_t)b * U + u) * T, rows.data() + ((size_t)u * B + b) * T, (size_t)T * 4);
    ts->score_B = B; ts->score_U = U; ts->score_T = T;
    m->stat_train_launches = ts->plan.launches;      // (statistic "train_persistent_launches", as a mode-0 step reports it)
    if (m->prof.on) m->prof.collect();
    return CASV_OK;
}

// The forward-only state a scoring call outside a session built (casv_score_targets); allowed when there is none.
extern "C" int casv_score_release(casv_model* m) {
    if (!m) return fail(CASV_ERR_ARG, "null argument");
    if (!m->score) return CASV_OK;
    release_state(m, m->score);
    m->score = nullptr;
    return CASV_OK;
}

// Outside a session the scoring call runs on a forward-only state of its own (m->score), built from the handle's committed weights
// and kept until they are committed anew; the phases find it where they find a session's state, in m->train, for the call's duration.
struct ScoreStateScope {
    casv_model* m; bool borrowed;
    ~ScoreStateScope() { if (borrowed) m->train = nullptr; }
};
static int score_state(casv_model* m) {
    if (m->score && m->score->commit_gen == m->commit_gen) return CASV_OK;
    (void)casv_score_release(m);
    if (m->W > 1024) return fail(CASV_ERR_ARG, "scoring supports width <= 1024");
    if (!m->committed) return fail(CASV_ERR_STATE, "casv_commit_weights must run first");
    TrainState* ts = new TrainState();
    ts->forward_only = true; ts->commit_gen = m->commit_gen;
    m->score = ts;
    if (int rc = build_state(m, ts, "")) { (void)casv_score_release(m); return rc; }
    return CASV_OK;
}

// The scoring call on Be sources with N given targets each (decoder row r = b * N + n reads source b's encoder pass): the range
// check over all rows before anything is launched, the state, at most two attempts.
static int score_call(casv_model* m, int32_t Be, int32_t N, int32_t T, int32_t U, int32_t A,
                      const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out, const ScoreOut& out) {
    if (!m || !enc_idx || !dec_in || !dec_out || !out.logp || !out.best || !out.rank || !out.nll || !out.count) return fail(CASV_ERR_ARG, "null argument");
    if (Be < 1 || N < 1 || T < 1 || U < 1 || A < 1 || (long long)Be * N > INT32_MAX) return fail(CASV_ERR_ARG, "bad shape");
    const int B = Be * N;
    const long long UB = (long long)U * B;
    for (long long i = 0; i < UB; ++i) {     // (before anything is launched)
        if (dec_out[i] < -1 || dec_out[i] >= m->V) return fail(CASV_ERR_ARG, "dec_out[%lld] = %d outside [-1, %d)", i, dec_out[i], m->V);
        if (dec_in[i] < -1 || dec_in[i] >= m->V) return fail(CASV_ERR_ARG, "dec_in[%lld] = %d outside [-1, %d)", i, dec_in[i], m->V);
    }
    HIPCHK(hipSetDevice(m->device));
    ScoreStateScope scope{m, false};
    if (!m->train) {
        if (int rc = score_state(m)) return rc;
        m->train = m->score; scope.borrowed = true;
    }
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_TRAIN));       // (the forward pass of a mode-0 step, in its arithmetic)
    OrderedScope ordered(m, m->deterministic);
    const std::vector<float> ones((size_t)UB, 1.0f);            // (stage_inputs stages the step's sample weights: the head reads none)
    Step s{};
    s.m = m; s.ts = m->train; s.st = m->stream;
    s.mode = 0; s.B = B; s.Be = Be; s.N = N; s.T = T; s.U = U; s.A = A;
    s.enc_idx = enc_idx; s.enc_val = enc_val; s.dec_in = dec_in; s.dec_out = dec_out; s.weights = ones.data();
    s.W = m->W; s.V = m->V; s.Vp = m->Vp; s.C = m->C; s.D = m->D;
    s.TB = (long long)T * Be; s.UB = UB;
    // (no masks, no regulariser; det / fused govern the backward pass and the ordered sums of the loss: the head has neither, and
    // persist_launch and the launchers read the "deterministic" option from the handle)
    s.training = false; s.det = false; s.fused = false;
    s.deep = m->cfg.deep_bidirectional_encoder != 0 && s.D >= 2;
    s.residual = m->cfg.residual_connections != 0; s.bridged = m->cfg.bridge_dense != 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool redo = false;
        if (int rc = score_attempt(s, out, &redo)) return rc;
        if (!redo) return CASV_OK;
    }
    return fail(CASV_ERR_STATE, "the scoring call gave up twice: its second attempt took a persistent launch");
}

extern "C" int casv_score_targets(casv_model* m, int32_t B, int32_t T, int32_t U, int32_t A,
                                  const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                                  float* logp, int32_t* best, int32_t* rank, double* nll, int32_t* count, float* align) {
    return score_call(m, B, 1, T, U, A, enc_idx, enc_val, dec_in, dec_out, ScoreOut{logp, best, rank, nll, count, align});
}

// N candidate targets per source on ONE encoder pass (kt:407 / s2s:491-497 as casv_score_targets, whose N = 1 call this is): the
// embedding, the encoder stack, its final states and u = enc_out . U_a are computed for the B sources; every decoder row -- the
// decoder layers, the attention cell, the projection, the head -- for the B * N candidates, row b * N + n on source b.
extern "C" int casv_score_candidates(casv_model* m, int32_t B, int32_t N, int32_t T, int32_t U, int32_t A,
                                     const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                                     float* logp, int32_t* best, int32_t* rank, double* nll, int32_t* count, float* align) {
    return score_call(m, B, N, T, U, A, enc_idx, enc_val, dec_in, dec_out, ScoreOut{logp, best, rank, nll, count, align});
}

extern "C" int casv_score_get_alignments_sparse(casv_model* m, int32_t K, int32_t* lo, float* w) {
    if (!m || !lo || !w) return fail(CASV_ERR_ARG, "null argument");
    TrainState* ts = m->train ? m->train : m->score;
    if (!ts || !ts->score_B) return fail(CASV_ERR_STATE, "no scoring call to take alignments from");
    if (K < 2 * m->cfg.window_width + 1 || K > 64) return fail(CASV_ERR_ARG, "K=%d: need at least 2*window_width+1 = %d weights per step (at most 64)", K, 2 * m->cfg.window_width + 1);
    HIPCHK(hipSetDevice(m->device));
    const size_t n = (size_t)ts->score_B * ts->score_U;
    if (int rc = ts->s_lo.ensure(n * 4)) return rc;
    if (int rc = ts->s_w.ensure(n * K * 4)) return rc;
    launch_score_extract_sparse(ts->Ast.as<float>(), ts->WIN.as<int>(), ts->score_B, ts->score_U, ts->score_T, K, ts->s_lo.as<int>(),
                                ts->s_w.as<float>(), m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(lo, ts->s_lo.p, n * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(w, ts->s_w.p, n * K * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}

// The K likeliest characters and the entropy of every position of the LAST scoring call: the logits of its B * U rows still lie in
// the state's buffer (the head writes nothing back into them), one launch reads them; nothing a later call reads is changed.
extern "C" int casv_score_get_alternatives(casv_model* m, int32_t K, int32_t* alt_idx, float* alt_logp, float* entropy) {
    if (!m) return fail(CASV_ERR_ARG, "null argument");
    if (K < 1 || K > m->V || K > 64) return fail(CASV_ERR_ARG, "K=%d outside [1, min(V, 64)] = [1, %d]", K, m->V < 64 ? m->V : 64);
    TrainState* ts = m->train ? m->train : m->score;
    if (!ts || !ts->score_B) return fail(CASV_ERR_STATE, "no scoring call to take alternatives from");
    if (!alt_idx || !alt_logp) return fail(CASV_ERR_ARG, "null argument");      // (after the state: a caller without a shape learns why)
    HIPCHK(hipSetDevice(m->device));
    const size_t n = (size_t)ts->score_B * ts->score_U;
    if (int rc = ts->s_alt_idx.ensure(n * K * 4)) return rc;
    if (int rc = ts->s_alt_logp.ensure(n * K * 4)) return rc;
    if (int rc = ts->s_entropy.ensure(n * 4)) return rc;
    launch_score_alternatives(ts->logits.as<float>(), ts->score_B, ts->score_U, m->V, m->Vp, K, ts->s_alt_idx.as<int>(),
                              ts->s_alt_logp.as<float>(), entropy ? ts->s_entropy.as<float>() : nullptr, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(alt_idx, ts->s_alt_idx.p, n * K * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(alt_logp, ts->s_alt_logp.p, n * K * 4, hipMemcpyDeviceToHost, m->stream));
    if (entropy) HIPCHK(hipMemcpyAsync(entropy, ts->s_entropy.p, n * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}

// Test support: the head alone on the caller's logits (R,V), laid out with the library's row stride and the padding filled.
extern "C" int casv_debug_score_rows(casv_model* m, int32_t R, int32_t V, const float* logits, const int32_t* target, float pad_value,
                                     float* logp, int32_t* best, int32_t* rank) {
    if (!m || !logits || !target || !logp || !best || !rank) return fail(CASV_ERR_ARG, "null argument");
    if (R < 1 || R > (1 << 20) || V < 1 || V > 4096) return fail(CASV_ERR_ARG, "R must be in [1, 2^20], V in [1, 4096]");
    HIPCHK(hipSetDevice(m->device));
    const int Vp = (V + 31) & ~31;           // (the library's row stride: engine.hip, casv_model_create)
    std::vector<float> x((size_t)R * Vp, pad_value);
    for (int r = 0; r < R; ++r) memcpy(&x[(size_t)r * Vp], logits + (size_t)r * V, (size_t)V * 4);
    DevBuf dx, dt, dl, db, dr;
    DebugBuffers release_on_exit{m->stream};
    if (int rc = dx.ensure(x.size() * 4)) return rc;
    for (DevBuf* b : {&dt, &dl, &db, &dr}) if (int rc = b->ensure((size_t)R * 4)) return rc;
    HIPCHK(hipMemcpyAsync(dx.p, x.data(), x.size() * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(dt.p, target, (size_t)R * 4, hipMemcpyHostToDevice, m->stream));
    launch_score_rows(dx.as<float>(), dt.as<int>(), R, 1, V, Vp, dl.as<float>(), db.as<int>(), dr.as<int>(), m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(logp, dl.p, (size_t)R * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(best, db.p, (size_t)R * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(rank, dr.p, (size_t)R * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}

// Test support: score_alternatives_kernel alone on the caller's logits (R,V), laid out as casv_debug_score_rows lays them out.
extern "C" int casv_debug_alternatives_rows(casv_model* m, int32_t R, int32_t V, int32_t K, const float* logits, float pad_value,
                                            int32_t* alt_idx, float* alt_logp, float* entropy) {
    if (!m || !logits || !alt_idx || !alt_logp) return fail(CASV_ERR_ARG, "null argument");
    if (R < 1 || R > (1 << 20) || V < 1 || V > 4096) return fail(CASV_ERR_ARG, "R must be in [1, 2^20], V in [1, 4096]");
    if (K < 1 || K > V || K > 64) return fail(CASV_ERR_ARG, "K=%d outside [1, min(V, 64)] = [1, %d]", K, V < 64 ? V : 64);
    HIPCHK(hipSetDevice(m->device));
    const int Vp = (V + 31) & ~31;
    std::vector<float> x((size_t)R * Vp, pad_value);
    for (int r = 0; r < R; ++r) memcpy(&x[(size_t)r * Vp], logits + (size_t)r * V, (size_t)V * 4);
    DevBuf dx, di, dl, de;
    DebugBuffers release_on_exit{m->stream};
    if (int rc = dx.ensure(x.size() * 4)) return rc;
    if (int rc = di.ensure((size_t)R * K * 4)) return rc;
    if (int rc = dl.ensure((size_t)R * K * 4)) return rc;
    if (int rc = de.ensure((size_t)R * 4)) return rc;
    HIPCHK(hipMemcpyAsync(dx.p, x.data(), x.size() * 4, hipMemcpyHostToDevice, m->stream));
    launch_score_alternatives(dx.as<float>(), R, 1, V, Vp, K, di.as<int>(), dl.as<float>(), entropy ? de.as<float>() : nullptr, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(alt_idx, di.p, (size_t)R * K * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(alt_logp, dl.p, (size_t)R * K * 4, hipMemcpyDeviceToHost, m->stream));
    if (entropy) HIPCHK(hipMemcpyAsync(entropy, de.p, (size_t)R * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}

// Test support: sample_kernel (cut == nullptr) or sample_cut_kernel alone on the caller's logits (R,V), laid out as
// casv_debug_score_rows lays them out.
static int debug_sample_rows(casv_model* m, int32_t R, int32_t V, const casv_sample_params* p, const casv_sample_cut* cut, int32_t step,
                             const int64_t* stream, const int32_t* sample, const float* logits, const float* u, float pad_value, int32_t* out_idx,
                             float* out_logp, float* out_logq, float* out_feedback) {
    if (!logits || !out_feedback) return fail(CASV_ERR_ARG, "null argument");
    if (!m || !p || !out_idx || !out_logp || !out_logq) return fail(CASV_ERR_ARG, "null argument");
    if (!(p->temperature > 0.f) || !(p->temperature < INFINITY)) return fail(CASV_ERR_ARG, "temperature=%g must be finite and positive", (double)p->temperature);
    if (p->top_k < 0 || p->top_k > 64) return fail(CASV_ERR_ARG, "top_k=%d out of range 0..64", p->top_k);
    if (R < 1 || R > (1 << 20) || V < 1 || V > 4096) return fail(CASV_ERR_ARG, "R must be in [1, 2^20], V in [1, 4096]");
    if (step < 0 || step >= 2 * CASV_MAX_T) return fail(CASV_ERR_ARG, "step=%d out of range 0..%d", step, 2 * CASV_MAX_T - 1);
    HIPCHK(hipSetDevice(m->device));
    if (cut && !sample_cut_ready()) return fail(CASV_ERR_HIP, "the runtime refused sample_cut_kernel's %d bytes of dynamic LDS", SAMPLE_CUT_LDS);
    const int Vp = (V + 31) & ~31;           // (the library's row stride: engine.hip, casv_model_create)
    std::vector<float> x((size_t)R * Vp, pad_value);
    for (int r = 0; r < R; ++r) memcpy(&x[(size_t)r * Vp], logits + (size_t)r * V, (size_t)V * 4);
    DebugBuffers bufs{m->stream};
    int rc = 0;
    SampleArgs a{};
    a.logits = static_cast<const float*>(bufs.put(x.data(), x.size(), rc)); if (rc) return rc;
    // (the output slot is step + 1 of a store whose slots all lie on the one (R,Vp) buffer)
    a.feedback = static_cast<float*>(bufs.put(nullptr, (size_t)R * Vp, rc)); if (rc) return rc;
    a.fb_slot = 0; a.R = R; a.V = V; a.step_imm = step; a.rows_per_line = 1;
    if (stream) { a.stream = static_cast<const long long*>(bufs.put(stream, (size_t)R * 2, rc)); if (rc) return rc; }
    if (sample) { a.sample = static_cast<const int*>(bufs.put(sample, (size_t)R, rc)); if (rc) return rc; }
    if (u) { a.u = static_cast<const float*>(bufs.put(u, (size_t)R, rc)); if (rc) return rc; }
    a.seed = p->seed; a.temperature = p->temperature; a.top_k = p->top_k;
    a.out_idx = static_cast<int*>(bufs.put(nullptr, (size_t)R, rc)); if (rc) return rc;
    a.out_logp = static_cast<float*>(bufs.put(nullptr, (size_t)R, rc)); if (rc) return rc;
    a.out_logq = static_cast<float*>(bufs.put(nullptr, (size_t)R, rc)); if (rc) return rc;
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
