// The training state: the step's packed tensors with their gradients and Adam moments, the layers' buffers, the step's scratch --
// and the table that says which Keras tensor lives where in the packed ones (keras_table.h).  A session's state hangs on the
// handle as m->train (train_state.hip), a scoring call's forward-only state as m->score (score.hip); train.hip runs the step on it.
#pragma once
#include "engine.h"
#include "keras_table.h"
#include "train_kernels.h"

namespace casv {

struct TTensor { std::string name; DevBuf w, g, m, v; size_t n = 0; bool frozen = false; };

struct TLayer {
    std::string name;
    int kx = 0, kr = 0, len = 0;
    int rows = 0;                          // rows per time step: the step's B, an encoder layer of a candidates call its Be sources (plan_buffers)
    bool reverse = false;
    bool encoder = false; int dir = 0;     // an encoder layer (else a decoder layer); direction 0 forward / 1 backward (keras_table.h)
    int iwx = -1, iwr = -1, ib = -1;
    DevBuf wxT, wrT;                       // derived: [kx][4W], [kr][4W]
    DevBuf Hown, Cs, Gt, Z, dRec;
    bool drec_cleared = false;             // this step's forward recurrence has cleared dRec (train_persist.hip: RecJob.zero)
    float* hs = nullptr; long long hs_ld = 0;
    TLayer() = default;
    TLayer(TLayer&&) noexcept = default; TLayer& operator=(TLayer&&) noexcept = default;
};

}  // namespace casv

struct TrainState {
    casv_adam_params ap{};
    long step = 0;
    std::vector<KerasEntry> table;         // the Keras view of tens (keras_table.h): built once by build_state
    std::vector<TTensor> tens;
    std::vector<TLayer> layers;            // enc1_fw, enc1_bw, enc2.., dec1..decD
    int iE = -1, iUT = -1, iWaT = -1, ibUW = -1, iva = -1, ibv = -1;
    DevBuf ETp, WaN, UaN;                  // derived: E^T padded [W][Vp], W_a [W][W], U_a [C][W]
    // bridge_dense (seq2seq.py:299-301): per encoder layer n (index n - 1) and state s (0 = h, 1 = c) the Dense kernel transposed
    // [W out][W in] (the B operand of the forward product), its bias, and -- derived -- the kernel as Keras holds it [W in][W out]
    // (the B operand of the data gradient); the bridged states, and the tanh' products of the backward pass
    struct Bridge {
        int ikt = -1, ib = -1; DevBuf kn;
        Bridge() = default;
        Bridge(Bridge&&) noexcept = default; Bridge& operator=(Bridge&&) noexcept = default;
    };
    std::vector<Bridge> bridge;            // [2 * (n - 1) + s]
    DevBuf hbr, cbr, brtmp, Ytop;          // [D][Be][W] bridged final states; scratch [Be][W]; residual_connections: top output + its input [U*B][W]
    DevBuf h0rep, c0rep;                   // casv_score_candidates, N > 1: the decoder's initial states [D][B][W], every source's rows N times
    int B = 0, T = 0, U = 0, A = 0;        // B: the step's batch = the decoder's rows
    int Be = 0, N = 1;                     // the encoder's lines and the decoder rows per line, Be * N == B (N > 1: casv_score_candidates only)
    DevBuf e_idx, e_val, d_in, d_out, d_w, m_enc, m_dec, m_cell;
    DevBuf d_gold, d_mix;                  // casv_train_step_sampled: the gold decoder input [B][U] (d_in holds the mix), every pass's mix [passes][B][U]
    std::vector<int32_t> h_mix;            // ... and ("deterministic") the last mix on the host, for the decoder's character segments
    DevBuf d_sidx, d_sq;                   // casv_train_step_soft: the soft targets' slots [B][U][K] (index, mass) in place of d_out
    DevBuf r_cost, r_coef, r_q, r_risk, r_parts;   // casv_train_step_risk: cost / coefficient / q [B], risk and its share of the loss [G] (logp: s_logp)
    DevBuf X0, H1, u, Y0, Ym, WQ, Ast, WIN, RecIn, logits, dG, d_enc, du, DWQ, DSrows, dhatt, dfin, dcbuf, dcbuf2, dX0, dXtop, dXl, dYl, dOin, dvaP, dbvP;
    std::vector<DevBuf> O, DO;             // masked layer outputs (encoder O[n], decoder DO[n])
    std::vector<DevBuf> XD;                // deep_bidirectional_encoder: layer n's input = the cross sum of O[n-1] (seq2seq.py:246-259)
    DevBuf loss, normsq;
    DevBuf dcalt;                          // second dL/dc buffers of the fused backward steps (two layers)
    // "deterministic" option: the ordered K-major contractions' partial sums, the workgroups' loss / norm parts, the per-character
    // segments of the embedding gradient (encoder, decoder input) and their host images
    int tn_ws_rc = 0;                      // the ordered contractions' workspace could not be had this step (its error, reported by the step)
    DevBuf tn_ws, sum_parts, seg_enc_off, seg_enc_pos, seg_dec_off, seg_dec_pos;
    std::vector<int> h_seg_enc_off, h_seg_enc_pos, h_seg_dec_off, h_seg_dec_pos;
    DevBuf rec_cnt; TrainStepPlan plan; int rec_checked = 0, rec_skip = 0, rec_penalty = 0;   // persistent recurrences: counters per launch, the step's launches, back-off
    const unsigned* rec_abort[TRAIN_LAUNCH_CAP] = {nullptr};    // ... and where each launch leaves its "gave up" word
    // The attention cell's backward recurrence as TWO launches side by side (train_persist_topb.hip, split_a): the second stream and
    // the events that tie it into the step; split_off: a step gave up with the two launches in flight -- one launch from then on.
    hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr; bool split_off = false; int split_launch = -1;
    // casv_score_targets: the head's results on the device in the caller's order -- logp / best / rank [B][U], nll / count [B], the
    // window form of the attention rows -- and whether the buffers hold a scoring call's attention rows (score_B x score_U x score_T).
    // forward_only: the state of a scoring call outside a session (m->score) -- weights in the train layout, the derived transposes,
    // the forward buffers; no gradient, no Adam moment, no backward buffer.  commit_gen: the commit of the handle's weights it holds.
    DevBuf s_logp, s_best, s_rank, s_nll, s_count, s_lo, s_w;
    DevBuf s_alt_idx, s_alt_logp, s_entropy;     // casv_score_get_alternatives: [B][U][K], [B][U] of the last retrieval
    int score_B = 0, score_U = 0, score_T = 0;
    bool forward_only = false; unsigned long long commit_gen = 0;
    float* W_(int i) { return tens[i].w.as<float>(); }
    float* G_(int i) { return tens[i].g.as<float>(); }
};

namespace casv {

// The handle's weights (Keras layout, m->host) as the step's packed tensors in ts, with the derived layouts: a session's state
// (with gradients and Adam moments) or, ts->forward_only, a scoring state.  On an error the caller releases ts.
int build_state(casv_model* m, TrainState* ts, const std::string& frozen_csv);
// Waits for the state's work, destroys its side stream and events, deletes it: every buffer frees itself.
void release_state(casv_model* m, TrainState* ts);
// Refresh the layouts derived from the master tensors (after set-up and after every update).
void refresh_derived(casv_model* m, TrainState* ts);

}  // namespace casv
