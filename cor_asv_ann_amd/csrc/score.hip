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
    Step s = step_view(m, StepArgs{0, B, T, U, A, enc_idx, enc_val, dec_in}, Be, N);
    s.dec_out = dec_out; s.weights = ones.data();
    // (no masks, no regulariser; det / fused govern the backward pass and the ordered sums of the loss: the head has neither, and
    // persist_launch and the launchers read the "deterministic" option from the handle)
    s.training = false; s.det = false; s.fused = false;
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
