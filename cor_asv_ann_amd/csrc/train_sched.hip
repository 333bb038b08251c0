// Scheduled sampling inside the train step, in its parallel form (Duckworth et al. 2019): the passes that
// casv_train_step_sampled runs between the step's phases 4 and 5 (train.hip), and the entry itself.
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
int check_sched_params(const casv_sched_params* p, bool with_passes) {
    if (!p) return fail(CASV_ERR_ARG, "null argument");
    if (!(p->ratio >= 0.f && p->ratio <= 1.f)) return fail(CASV_ERR_ARG, "ratio=%g outside [0, 1]", (double)p->ratio);
    if (with_passes && (p->passes < 1 || p->passes > 8)) return fail(CASV_ERR_ARG, "passes=%d outside 1..8", p->passes);
    if (p->pick != 0 && p->pick != 1) return fail(CASV_ERR_ARG, "pick=%d: 0 (greedy) or 1 (sample)", p->pick);
    if (p->pick == 1 && (!(p->temperature > 0.f) || !(p->temperature < INFINITY)))
        return fail(CASV_ERR_ARG, "temperature=%g must be finite and positive", (double)p->temperature);
    return CASV_OK;
}

// ... and of a cut beside them: only the sampled pick can be cut
int check_sched_cut(const casv_sched_params* p, const casv_sample_cut* cut) {
    if (int rc = check_sample_cut(cut)) return rc;
    if (p->pick == 0 && (cut->top_k != 0 || cut->top_p != 1.f)) return fail(CASV_ERR_ARG, "a cut (top_k=%d, top_p=%g) needs pick 1 (sample)", cut->top_k, (double)cut->top_p);
    return CASV_OK;
}

// The step behind casv_train_step_sampled (cut == nullptr) and casv_train_step_sampled_cut.  It refuses in an order of its own: what
// scheduled sampling adds first, then -- behind the hand-over of a step without a pass -- what every step entry refuses.
static int train_step_sampled(casv_model* m, const StepArgs& a, const int32_t* dec_out, const casv_sched_params* p, const casv_sample_cut* cut,
                              int32_t* out_dec_in) {
    static const char* const modes = "mode must be 1 (train) or 2 (gradients only): validation stays teacher-forced";
    if (!m || !a.dec_in || !out_dec_in) return fail(CASV_ERR_ARG, "null argument");
    if (int rc = check_sched_params(p, true)) return rc;
    if (int rc = cut ? check_sched_cut(p, cut) : 0) return rc;
    if (a.mode != 1 && a.mode != 2) return fail(CASV_ERR_ARG, "%s", modes);
    if (a.B < 1 || a.U < 1) return fail(CASV_ERR_ARG, "bad shape");
    if (p->ratio == 0.f) {              // no pass: casv_train_step's launches and bits, every slice the gold input
        if (int rc = casv_train_step(m, a.mode, a.B, a.T, a.U, a.A, a.enc_idx, a.enc_val, a.dec_in, dec_out, a.weights, a.mask_enc, a.mask_dec,
                                     a.mask_cell, a.loss_out, a.norm_out))
            return rc;
        for (int q = 0; q < p->passes; ++q) memcpy(out_dec_in + (size_t)q * a.B * a.U, a.dec_in, (size_t)a.B * a.U * 4);
        return CASV_OK;
    }
    if (int rc = check_step_args(m, a, dec_out, 1, modes)) return rc;
    return run_step(m, a, [&](Step& s) {
        if (cut && !sched_mix_cut_ready()) return fail(CASV_ERR_HIP, "the runtime refused sched_mix_cut_kernel's %d bytes of dynamic LDS", SAMPLE_CUT_LDS);
        s.dec_out = dec_out; s.sched = p; s.mix_out = out_dec_in; s.cut = cut;
        return 0;
    });
}

extern "C" int casv_train_step_sampled(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                                       const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                                       const float* weights, const float* mask_enc, const float* mask_dec, const float* mask_cell,
                                       const casv_sched_params* p, int32_t* out_dec_in, double* loss_out, double* norm_out) {
    return train_step_sampled(m, StepArgs{mode, B, T, U, A, enc_idx, enc_val, dec_in, weights, mask_enc, mask_dec, mask_cell, loss_out, norm_out},
                              dec_out, p, nullptr, out_dec_in);
}

extern "C" int casv_train_step_sampled_cut(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                                           const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                                           const float* weights, const float* mask_enc, const float* mask_dec, const float* mask_cell,
                                           const casv_sched_params* p, const casv_sample_cut* cut, int32_t* out_dec_in, double* loss_out,
                                           double* norm_out) {
    if (!cut) return fail(CASV_ERR_ARG, "null argument");
    return train_step_sampled(m, StepArgs{mode, B, T, U, A, enc_idx, enc_val, dec_in, weights, mask_enc, mask_dec, mask_cell, loss_out, norm_out},
                              dec_out, p, cut, out_dec_in);
}
