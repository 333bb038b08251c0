// One attempt's view of the train step (Step) and the phases a scoring call shares with it (train.hip defines them, score.hip
// runs the first four and the projection in front of its own head).
#pragma once
#include "train_state.h"
#include <functional>

namespace casv {

// One attempt's view of the step: what the caller passed, the model's shapes, the step's flags, and what one phase leaves for the
// next.  casv_train_step fills the first three groups once; every attempt starts from a copy and its phases fill in the rest.
struct Step {
    casv_model* m; TrainState* ts; hipStream_t st;
    int mode, B, T, U, A;           // B: the step's batch, the decoder's rows
    int Be, N;                      // the encoder's lines, decoder rows per line: Be * N == B (casv_train_step: Be = B, N = 1)
    const int32_t* enc_idx; const float* enc_val; const int32_t* dec_in; const int32_t* dec_out; const float* weights;
    const float* mask_enc; const float* mask_dec; const float* mask_cell;
    int K; const int32_t* soft_idx; const float* soft_q;      // casv_train_step_soft: K > 0, (B,U,K) slots in place of dec_out (nullptr)
    int RN; const float* cost; double alpha, inv_groups;     // casv_train_step_risk: RN > 0 candidates per group, cost (B), 1 / max(groups with a member, 1)
    const casv_sched_params* sched; int32_t* mix_out;         // casv_train_step_sampled with ratio > 0: the passes' parameters, (passes,B,U) out
    const casv_sample_cut* cut;     // casv_train_step_sampled_cut: the cut of the sampled pick (nullptr: none)
    int W, V, Vp, C, D;
    long long TB, UB;
    // "deterministic": every sum of the step in a fixed order -- the per-step launch forms only (no persistent
    // recurrence, hence no give-up fallback; no fused backward step), no split-K in the launcher, the K-major contractions'
    // shares added in order, the workgroups' loss / norm parts added by one ordered pass, the embedding gradient per character
    bool training, det, fused, deep, residual, bridged;
    // plan_buffers: the encoder's final states [n-1][Be][W], the decoder's initial states [n-1][B][W] (the bridged ones with
    // bridge_dense; N > 1: either, every row N times), the
    // gradients w.r.t. the final states [n-1][0|1][B][W], the ordered sums' parts (deterministic only)
    float* hfin; float* cfin; const float* h0base; const float* c0base; float* dfin; double* parts;
    // stage_inputs: the dropout masks on the device (nullptr: none) -- enc = 2W + (D-1)*W floats (deep: D * 2W), dec = (D-1)*W floats,
    // cell = B*(W+C) -- and 1 / the number of weighted targets
    const float* menc; const float* mdec; const float* mcell; float inv_count;
    // forward_layers: the cell's input sequence (decoder layer D - 1's masked outputs, Y0 when D == 1) and the attended sequence O[D]
    const float* y; const float* enc_out;
    // loss_head: the projection's input
    const float* proj_in; long long proj_ld;

    const float* menc_n(int n) const { return menc ? menc + (n == 1 ? 0 : deep ? (n - 1) * 2 * W : 2 * W + (n - 2) * W) : nullptr; }   // layer n (1-based)
    const float* mdec_n(int n) const { return mdec ? mdec + (n - 1) * W : nullptr; }
    TLayer& enc_layer(int n) const { return ts->layers[n]; }            // n >= 2 -> index n (not with a deep bidirectional encoder)
    TLayer& enc_dir(int n, int dir) const { return ts->layers[2 * (n - 1) + dir]; }      // deep: layer n = 1..D, direction 0 fw / 1 bw
    TLayer& dec_layer(int n) const { return ts->layers[(deep ? 2 * D - 1 : D) + n]; }    // n = 1..D
    TLayer& top() const { return dec_layer(D); }                        // the attention cell
    const float* dec_h0(int n) const { return h0base + (size_t)(n - 1) * B * W; }        // decoder layer n starts from encoder layer n's final state
    const float* dec_c0(int n) const { return c0base + (size_t)(n - 1) * B * W; }
    float* dfin_h(int n) const { return dfin + (size_t)(2 * (n - 1)) * B * W; }
    float* dfin_c(int n) const { return dfin + (size_t)(2 * (n - 1) + 1) * B * W; }
    bool res_top() const { return residual && D >= 2; }                 // the projection reads the cell's outputs PLUS its input sequence
};

// The phases (train.hip), each on the state the phases before it left; 0 or an error.
int plan_buffers(Step& s);          // 1: every buffer large enough for the step's shapes, the layers' output places
int stage_inputs(Step& s);          // 2: batch, masks, segments on the device; sums, counters, gradients cleared
int forward_layers(Step& s);        // 3: encoder stack beside the decoder layers below the cell; final states, bridges, u
int forward_cell(Step& s);          // 4: the attention cell
int projection(Step& s);            // the tied output projection: s.proj_in, the logits [U*B][Vp]
int decoder_layer_alone(Step& s, int k, const float* y);      // decoder layer k < D alone in its launch on the input sequence y: DO[k]
int sched_passes(Step& s);          // between 4 and 5, casv_train_step_sampled only (train_sched.hip): the passes of scheduled sampling
// per-character segments of an index array [B][L][A_] for the ordered embedding gradient ("deterministic")
void char_segments(const int32_t* idx, int B, int L, int A_, int V, std::vector<int>& off, std::vector<int>& pos);
// One attempt at the step, the phases in order; *redo: a persistent recurrence gave up, the caller starts over.
int train_attempt(Step s, double* loss_out, double* norm_out, bool* redo);

// What every step entry takes from its caller, as the C ABI names it (B: the step's batch).
struct StepArgs {
    int32_t mode, B, T, U, A;
    const int32_t* enc_idx; const float* enc_val; const int32_t* dec_in; const float* weights;
    const float* mask_enc; const float* mask_dec; const float* mask_cell;
    double* loss_out; double* norm_out;
};
// The view of Be lines with N decoder rows each that an entry hands an attempt (the targets are the entry's to add).
Step step_view(casv_model* m, const StepArgs& a, int Be, int N);
// The step entries' common refusals and common body (train.hip): fill adds the entry's fields to the view, done (if any) takes what
// the entry hands back beside loss and norm from the attempt that finished; either returns 0 or the error the call ends with.
using StepHook = std::function<int(Step&)>;
int check_step_args(const casv_model* m, const StepArgs& a, bool own_pointers, int min_mode, const char* mode_message);
int run_step(casv_model* m, const StepArgs& a, const StepHook& fill, const StepHook& done = nullptr);
int recurrences_gave_up(casv_model* m, bool& any);      // did a persistent recurrence so far give up?  (then nothing has been updated)

}  // namespace casv

// The rules of an entry's own arguments, which its head's test entry (debug_rows.hip) checks as the entry does
int check_soft_targets(long long positions, int K, int V, const int32_t* soft_idx, const float* soft_q);   // train.hip
int check_risk(int B, int N, const float* cost, double alpha, double* inv);
int check_sched_params(const casv_sched_params* p, bool with_passes);                                      // train_sched.hip
int check_sched_cut(const casv_sched_params* p, const casv_sample_cut* cut);
