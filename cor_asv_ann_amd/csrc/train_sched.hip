// Scheduled sampling inside the train step, in its parallel form (Duckworth et al. 2019): the passes that
// casv_train_step_sampled runs between the step's phases 4 and 5 (train.hip), the entry itself and the mix kernel's test entry.
// The passes add no launch site of their own: the decoder layers and the cell run again through train.hip's own phase functions,
// so every persistent launch of a pass is planned, counted and checked for a give-up where the teacher-forced ones are.
#include "train_step.h"
#include <cstring>

using namespace casv;

namespace casv {

// Between phases 4 and 5 of a step with ratio > 0: per pass the logits of the current tape, the mix
// (sched_kernels.hip) into d_in and the pass's slice of d_mix, Y0 again from d_in, the decoder layers below the cell again, each alone,
// and the cell again.  The encoder layers, u and the final / bridged states stand as phase 3 left them.  Leaves what phases 3 and 4
// leave for the decoder, on the last mix; every pass's mix on its way to the caller; (deterministic) the decoder's character
// segments of the last mix on the device, which takes a wait for the stream.
int sched_passes(Step& s) {
    casv_model* m = s.m; TrainState* ts = s.ts; hipStream_t st = s.st;
    const int B = s.B, U = s.U, W = s.W, V = s.V, D = s.D;
    const long long UB = s.UB;
    const casv_sched_params& sp = *s.sched;
    for (int p = 0; p < sp.passes; ++p) {
        if (int rc = projection(s)) return rc;
        SchedMixArgs a{};
        a.logits = ts->logits.as<float>(); a.gold = ts->d_gold.as<int>(); a.d_in = ts->d_in.as<int>(); a.out = ts->d_mix.as<int>() + (long long)p * UB;
        a.R = UB; a.B = B; a.U = U; a.V = V; a.Vp = s.Vp;
        a.seed = sp.seed; a.step_id = sp.step_id; a.ratio = sp.ratio; a.temperature = sp.temperature; a.pick = sp.pick;
        if (s.cut) { a.top_k = s.cut->top_k; a.top_p = s.cut->top_p; }
        hipEvent_t ev{};
        m->prof_begin(PC_SAMPLE, 4.0 * (double)UB * V, 4.0 * (double)UB * V, ev);
        launch_sched_mix(a, st);
        m->prof_end(PC_SAMPLE, ev);
        launch_embed_tm(ts->W_(ts->iE), ts->d_in.as<int>(), nullptr, ts->Y0.as<float>(), B, U, 1, V, W, st);
        const float* y = ts->Y0.as<float>();
        for (int k = 1; k < D; ++k) {
            if (int rc = decoder_layer_alone(s, k, y)) return rc;
            y = ts->DO[k].as<float>();
        }
        s.y = y;
        if (int rc = forward_cell(s)) return rc;
    }
    HIPCHK(hipMemcpyAsync(s.mix_out, ts->d_mix.p, (size_t)sp.passes * UB * 4, hipMemcpyDeviceToHost, st));
    if (s.det) {
        ts->h_mix.resize((size_t)UB);
        HIPCHK(hipMemcpyAsync(ts->h_mix.data(), ts->d_in.p, UB * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        char_segments(ts->h_mix.data(), B, U, 1, V, ts->h_seg_dec_off, ts->h_seg_dec_pos);
        HIPCHK(hipMemcpyAsync(ts->seg_dec_off.p, ts->h_seg_dec_off.data(), (size_t)(V + 1) * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ts->seg_dec_pos.p, ts->h_seg_dec_pos.data(), ts->h_seg_dec_pos.size() * 4, hipMemcpyHostToDevice, st));
    }
    return 0;
}

}  // namespace casv

// Scheduled sampling's rules (include/cor_asv_ann_hip.h), checked before anything is launched or cleared.
static int check_sched_params(const casv_sched_params* p, bool with_passes) {
    if (!p) return fail(CASV_ERR_ARG, "null argument");
    if (!(p->ratio >= 0.f && p->ratio <= 1.f)) return fail(CASV_ERR_ARG, "ratio=%g outside [0, 1]", (double)p->ratio);
    if (with_passes && (p->passes < 1 || p->passes > 8)) return fail(CASV_ERR_ARG, "passes=%d outside 1..8", p->passes);
    if (p->pick != 0 && p->pick != 1) return fail(CASV_ERR_ARG, "pick=%d: 0 (greedy) or 1 (sample)", p->pick);
    if (p->pick == 1 && (!(p->temperature > 0.f) || !(p->temperature < INFINITY)))
        return fail(CASV_ERR_ARG, "temperature=%g must be finite and positive", (double)p->temperature);
    return CASV_OK;
}

// ... and of a cut beside them: only the sampled pick can be cut
static int check_sched_cut(const casv_sched_params* p, const casv_sample_cut* cut) {
    if (int rc = check_sample_cut(cut)) return rc;
    if (p->pick == 0 && (cut->top_k != 0 || cut->top_p != 1.f)) return fail(CASV_ERR_ARG, "a cut (top_k=%d, top_p=%g) needs pick 1 (sample)", cut->top_k, (double)cut->top_p);
    return CASV_OK;
}

// the step behind casv_train_step_sampled (cut == nullptr) and casv_train_step_sampled_cut
static int train_step_sampled(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                              const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                              const float* weights, const float* mask_enc, const float* mask_dec, const float* mask_cell,
                              const casv_sched_params* p, const casv_sample_cut* cut, int32_t* out_dec_in, double* loss_out, double* norm_out) {
    if (!m || !dec_in || !out_dec_in) return fail(CASV_ERR_ARG, "null argument");
    if (int rc = check_sched_params(p, true)) return rc;
    if (int rc = cut ? check_sched_cut(p, cut) : 0) return rc;
    if (mode != 1 && mode != 2) return fail(CASV_ERR_ARG, "mode must be 1 (train) or 2 (gradients only): validation stays teacher-forced");
    if (B < 1 || U < 1) return fail(CASV_ERR_ARG, "bad shape");
    if (p->ratio == 0.f) {              // no pass: casv_train_step's launches and bits, every slice the gold input
        if (int rc = casv_train_step(m, mode, B, T, U, A, enc_idx, enc_val, dec_in, dec_out, weights, mask_enc, mask_dec, mask_cell, loss_out, norm_out))
            return rc;
        for (int q = 0; q < p->passes; ++q) memcpy(out_dec_in + (size_t)q * B * U, dec_in, (size_t)B * U * 4);
        return CASV_OK;
    }
    if (!enc_idx || !dec_out || !weights || !loss_out) return fail(CASV_ERR_ARG, "null argument");
    if (!m->train) return fail(CASV_ERR_STATE, "casv_train_begin must run first");
    if (T < 1 || A < 1) return fail(CASV_ERR_ARG, "bad shape");
    HIPCHK(hipSetDevice(m->device));
    if (cut && !sched_mix_cut_ready()) return fail(CASV_ERR_HIP, "the runtime refused sched_mix_cut_kernel's %d bytes of dynamic LDS", SAMPLE_CUT_LDS);
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_TRAIN));
    OrderedScope ordered(m, m->deterministic);
    Step s = step_view(m, mode, B, T, U, A, enc_idx, enc_val, dec_in, weights, mask_enc, mask_dec, mask_cell);
    s.dec_out = dec_out; s.sched = p; s.mix_out = out_dec_in; s.cut = cut;
    // (a persistent launch of a pass that gave up is seen by the step's own checks: the second attempt takes per-step launches only)
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool redo = false;
        if (int rc = train_attempt(s, loss_out, norm_out, &redo)) return rc;
        if (!redo) return CASV_OK;
    }
    return fail(CASV_ERR_STATE, "the train step gave up twice: its second attempt took a persistent launch");
}

extern "C" int casv_train_step_sampled(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                                       const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                                       const float* weights, const float* mask_enc, const float* mask_dec, const float* mask_cell,
                                       const casv_sched_params* p, int32_t* out_dec_in, double* loss_out, double* norm_out) {
    return train_step_sampled(m, mode, B, T, U, A, enc_idx, enc_val, dec_in, dec_out, weights, mask_enc, mask_dec, mask_cell, p, nullptr,
                              out_dec_in, loss_out, norm_out);
}

extern "C" int casv_train_step_sampled_cut(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                                           const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                                           const float* weights, const float* mask_enc, const float* mask_dec, const float* mask_cell,
                                           const casv_sched_params* p, const casv_sample_cut* cut, int32_t* out_dec_in, double* loss_out,
                                           double* norm_out) {
    if (!cut) return fail(CASV_ERR_ARG, "null argument");
    return train_step_sampled(m, mode, B, T, U, A, enc_idx, enc_val, dec_in, dec_out, weights, mask_enc, mask_dec, mask_cell, p, cut,
                              out_dec_in, loss_out, norm_out);
}

// Test support: the mix kernel (under the cut, if given) alone on the caller's rows (R,V), laid out as casv_debug_score_rows lays them out.
static int debug_sched_rows(casv_model* m, int32_t R, int32_t V, const casv_sched_params* p, const casv_sample_cut* cut, const int32_t* b,
                            const int32_t* u, const float* logits, const int32_t* gold, float pad_value, int32_t* out) {
    if (!m || !b || !u || !logits || !gold || !out) return fail(CASV_ERR_ARG, "null argument");
    if (int rc = check_sched_params(p, false)) return rc;
    if (int rc = cut ? check_sched_cut(p, cut) : 0) return rc;
    if (R < 1 || R > (1 << 20) || V < 1 || V > 4096) return fail(CASV_ERR_ARG, "R must be in [1, 2^20], V in [1, 4096]");
    HIPCHK(hipSetDevice(m->device));
    if (cut && !sched_mix_cut_ready()) return fail(CASV_ERR_HIP, "the runtime refused sched_mix_cut_kernel's %d bytes of dynamic LDS", SAMPLE_CUT_LDS);
    const int Vp = (V + 31) & ~31;
    std::vector<float> x((size_t)R * Vp, pad_value);
    for (int r = 0; r < R; ++r) memcpy(&x[(size_t)r * Vp], logits + (size_t)r * V, (size_t)V * 4);
    DebugBuffers bufs{m->stream};
    int rc = 0;
    SchedMixArgs a{};
    a.logits = static_cast<const float*>(bufs.put(x.data(), x.size(), rc)); if (rc) return rc;
    a.gold = static_cast<const int*>(bufs.put(gold, (size_t)R, rc)); if (rc) return rc;
    a.row_b = static_cast<const int*>(bufs.put(b, (size_t)R, rc)); if (rc) return rc;
    a.row_u = static_cast<const int*>(bufs.put(u, (size_t)R, rc)); if (rc) return rc;
    a.out = static_cast<int*>(bufs.put(nullptr, (size_t)R, rc)); if (rc) return rc;
    a.R = R; a.B = R; a.U = 1; a.V = V; a.Vp = Vp;
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
