/*
 * cor_asv_ann_hip.h -- C ABI of the MI355X-native hot path of cor-asv-ann.
 *
 * The reference has no FFI: its hot path sits behind the Python class
 * ocrd_cor_asv_ann/lib/seq2seq.py:13 `Sequence2Sequence`, which crosses into the
 * Keras/TensorFlow runtime at `predict_on_batch` / `train_on_batch`.  This header is the
 * boundary a maintainer binds (ctypes) in place of those crossings.
 * Each entry point names the reference call site(s) it replaces.
 *
 * Conventions: every function returns 0 on success and a negative casv_status otherwise;
 * the message is available from casv_last_error() (thread-local).  The caller owns all
 * host buffers (C-contiguous, float32 / int32 / float64 as declared); the library owns
 * all device memory and its HIP stream.
 *
 * Limits (CASV_ERR_ARG beyond them; the reference itself has none but host memory): depth 1..8, width a
 * multiple of 32, vocabulary 2..4096, line length T <= 4096 positions (decode steps S <= 2T <= 8192),
 * hypotheses per line and step (batch_size) <= 1024, beam_width_in >= 1 (values above the vocabulary size act like
 * the vocabulary size), at most 64 results per line, and S * batch_size * (min(beam_width_in, V) + 1) < 2^31
 * hypotheses per line.  A search keeps every expansion's state on the device: casv_decode_beam needs about
 * 2T * batch_size * ((8 * depth + 4) * width + 4 * (V + T) + 60 * (beam_width_in + 1)) bytes per line
 * (CASV_ERR_NOMEM if the device cannot hold them -- decode fewer lines per call; the Python facade does that).  A handle is bound to one HIP device and is not
 * thread-safe (the reference runs single-threaded: wrapper/transcode.py:46 max_workers=1).
 * No C++ exceptions and no callbacks cross this boundary.
 */
#ifndef COR_ASV_ANN_HIP_H
#define COR_ASV_ANN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    CASV_OK = 0,
    CASV_ERR_ARG = -1,      /* bad argument / unsupported topology */
    CASV_ERR_STATE = -2,    /* call order (e.g. decode before encode) */
    CASV_ERR_HIP = -3,      /* HIP runtime failure */
    CASV_ERR_NOMEM = -4,
    CASV_ERR_NAN = -5       /* numpy would have raised "All-NaN slice" (seq2seq.py:1329,1335) */
} casv_status;

/* Topology of seq2seq.py:108-157.  residual_connections (seq2seq.py:284-291, 359-360), bridge_dense (seq2seq.py:299-301) and
 * deep_bidirectional_encoder (seq2seq.py:246-281) are built: encoder layers >= 3 hand on LSTM output + input sequence; the final
 * h / c of every encoder layer pass through Dense(width, tanh) layers "bridge<n>_h_K|b", "bridge<n>_c_K|b" ((W,W) kernel, (W) bias)
 * on their way to the decoder; with a deep bidirectional encoder EVERY encoder layer n is a BiLSTM ("enc<n>_fw_K|R|b",
 * "enc<n>_bw_K|R|b", kernels (2W,4W) for n >= 2) that reads the reference Lambda's "cross sum" of the layer below -- features 2k and
 * 2k+1 of [fw | bw] both replaced by their sum -- and hands on its backward final state; the attended width is then 2 * width for
 * every depth (att_U (2W,W), top decoder kernel (3W,4W)).  The train step adds the training graph's decoder sums (layers >= 2 and
 * the projection's input) -- which the reference's inference decoder does not have (seq2seq.py:421-436), restated as it is.
 * lm (lm_loss / lm_predict set at model build) and stateful must be 0 (both published models use the default topology,
 * wrapper/ocrd-tool.json:61-74).  The LM output of lm_predict needs no other weights: it is a decode-time switch of the handle,
 * casv_set_option(m, "lm_predict", 1), read by casv_decode_beam, and casv_decoder_step_lm computes it for one step. */
typedef struct {
    int32_t depth;          /* seq2seq.py:117 */
    int32_t width;          /* seq2seq.py:115; must be a multiple of 32 (any other width: pad with dead units, as
                             * cor_asv_ann_amd/engine.py does -- all-zero weights keep a unit at h = c = 0, exactly) */
    int32_t voc_size;       /* seq2seq.py:123 */
    int32_t window_width;   /* attention.py:515, seq2seq.py:347 (5) */
    int32_t residual_connections, deep_bidirectional_encoder, bridge_dense, lm, stateful;
} casv_config;

/* Beam parameters of seq2seq.py:159-169 plus the constants of :1389-1397. */
typedef struct {
    int32_t batch_size;          /* N hypotheses per line per step (seq2seq.py:1414) */
    int32_t beam_width_in;       /* seq2seq.py:164 */
    int32_t beam_width_out;      /* seq2seq.py:169 */
    int32_t max_results;         /* how many finished hypotheses to return per line (>=1) */
    double  beam_threshold_in;   /* seq2seq.py:167 */
    double  rejection_threshold; /* seq2seq.py:162 */
    double  cost0;               /* seq2seq.py:1394 (3.0) */
} casv_beam_params;

typedef struct casv_model casv_model;

const char* casv_last_error(void);
int casv_device_count(void);
const char* casv_version(void);

/* Sequence2Sequence.configure() (seq2seq.py:190-489): allocate the weight set on a device. */
int casv_model_create(const casv_config* cfg, int device_id, casv_model** out);
void casv_model_destroy(casv_model* m);

/* Keras set_weights/get_weights per tensor (seq2seq.py:1172, 509-523).  Names and shapes are
 * those of SURVEY.md A.2: "E" (V,W); "enc1_fw_K|R|b", "enc1_bw_K|R|b"; "enc<n>_K|R|b";
 * "att_U" (C,W); "dec<n>_K|R|b"; "att_Wa" (W,W), "att_va" (W), "att_bUW" (W), "att_bv" (1); with bridge_dense also
 * "bridge<n>_h_K" (W,W), "bridge<n>_h_b" (W), "bridge<n>_c_K", "bridge<n>_c_b" for n = 1..depth (Keras Dense: y = x.K + b).
 * Layout is Keras': kernels (in,4W) with gate blocks i,f,c,o; row-major float32. */
int casv_set_weight(casv_model* m, const char* name, const float* data, int64_t count);
int casv_get_weight(casv_model* m, const char* name, float* out, int64_t capacity);
/* _resync_decoder() (seq2seq.py:526-528): repack the named tensors into the kernel layouts. */
int casv_commit_weights(casv_model* m);

/* encoder_model.predict_on_batch (seq2seq.py:403-406, 811, 1231).
 * Input is the sparse form of vectorize_lines' (B,T,V) array (seq2seq.py:1059-1093): per
 * position up to A (index, value) pairs, index < 0 = empty slot; a position with no pairs
 * is true-zero padding.  src_rej[b*T+t] = argmax of that input row or -1 if it is all zero
 * (what seq2seq.py:1458-1462 reads back during the beam search).
 * Leaves enc_out, u = attention_dense(enc_out) and the initial decoder states on the device. */
int casv_encode(casv_model* m, int32_t B, int32_t T, int32_t A,
                const int32_t* idx, const float* val, const int32_t* src_rej);
/* Copy the encoder outputs back (parity tests; mirrors the list encoder_model returns):
 * enc_out (B,T,C); states (2*depth, B, W) ordered h1,c1,...,hd,cd.  Either may be NULL. */
int casv_get_encoder_outputs(casv_model* m, float* enc_out, float* states);

/* The `encoder_outputs=` argument of decode_sequence_greedy / decode_sequence_beam (seq2seq.py:1305-1308,1382-1386) and
 * the `attention_input` + state inputs of decoder_model (seq2seq.py:470-473): install encoder outputs computed elsewhere
 * instead of running the encoder.  enc_out (B,T,C); states (2*depth, B, W) ordered h1,c1,...,hd,cd; a0 (B,T) initial
 * alignment or NULL for zeros (what the encoder returns, seq2seq.py:307-309); src_rej as in casv_encode or NULL. */
int casv_set_encoder_outputs(casv_model* m, int32_t B, int32_t T, const float* enc_out, const float* states,
                             const float* a0, const int32_t* src_rej);

/* One decoder_model.predict_on_batch (seq2seq.py:477-480, 1245, 1321, 1428) on explicit
 * inputs, for parity tests: R rows, `line[r]` selects the encoded line each row attends to.
 * p_in (R,V); states_in (2*depth, R, W) + a_in (R,T)  ->  probs (R,V), states_out, a_out. */
int casv_decoder_step(casv_model* m, int32_t R, const int32_t* line,
                      const float* p_in, const float* states_in, const float* a_in,
                      float* probs, float* states_out, float* a_out);

/* decoder_model.predict_on_batch with lm_predict (seq2seq.py:464-473): casv_decoder_step (same arguments, same results bit for bit)
 * plus lm_probs (R,V) = the decoder's context-free language model -- the top cell once more on the same input and states with zero
 * attention constants (enc_out = u = 0: a zero context, or NaN where the window is empty or the energy exp(tanh(q).v_a + b_v) is 0
 * or infinite: the whole row is NaN then), its states discarded, through the tied projection and softmax.  Always computed,
 * whatever the "lm_predict" option says; arithmetic 0 like casv_decoder_step. */
int casv_decoder_step_lm(casv_model* m, int32_t R, const int32_t* line,
                         const float* p_in, const float* states_in, const float* a_in,
                         float* probs, float* states_out, float* a_out, float* lm_probs);

/* decode_batch_greedy (seq2seq.py:1215-1286; mode 0: argmax without index 0, S = 2T steps for
 * all lines) and decode_sequence_greedy for every line at once (seq2seq.py:1288-1354; mode 1:
 * argmax over all V with the index-0 NaN write-back, a line's steps after its '\n' are not
 * reported).  out_idx/out_prob (B,S); out_len (B) = reported steps per line (mode 0: S);
 * out_align (B,S,T) or NULL.
 * A row whose candidates are all NaN: mode 0 reports index 1 with a NaN probability at that step and returns CASV_OK (the other
 * rows are untouched); mode 1 reports the same, ends the line there and returns CASV_ERR_NAN if that is before the line's '\n'
 * (the outputs are filled either way). */
int casv_decode_greedy(casv_model* m, int32_t mode, int32_t S,
                       int32_t* out_idx, float* out_prob, int32_t* out_len, float* out_align);

/* decode_sequence_beam (seq2seq.py:1356-1544) for all encoded lines at once.
 * For result k < max_results of line b: out_idx/out_prob ((B*max_results), S) characters and
 * probabilities, out_len length (incl. the final '\n'), out_score = cum_cost/(length-1)
 * (seq2seq.py:1543), out_rej ((B*max_results), S) = source position if that step was a
 * rejection candidate (one-hot alignment row, seq2seq.py:1495) else -1, out_align
 * ((B*max_results), S, T) or NULL.  n_found (B) = finished hypotheses per line (0 = the
 * generator would raise StopIteration, seq2seq.py:826); n_steps (B) = search iterations run.
 * With the option "lm_predict" = 1 (casv_set_option, read at every call) a child's cost -- and so cum_cost, the queue order, the
 * stopping test and out_score -- is -log of the LM's probability of its character (casv_decoder_step_lm), and a child whose LM
 * probability is NaN is dropped (seq2seq.py:1487-1490, 1503-1505); out_prob, the rejection candidates, the beam width, the order of
 * the children and the fed-back scores stay the decoder's.  Needs batch_size * ((2 * width + V) * 4 + 4 * (beam_width_in + 1)) more
 * bytes per line (per-step scratch of the LM). */
int casv_decode_beam(casv_model* m, const casv_beam_params* p, int32_t S,
                     int32_t* out_idx, float* out_prob, int32_t* out_len, double* out_score,
                     int32_t* out_rej, float* out_align, int32_t* n_found, int32_t* n_steps);

/* Sampling: `samples` lines DRAWN from the decoder for every encoded line, on one encoder pass.
 * Row r = b * samples + n steps in lockstep with all others for S steps; at step s it draws index v from the candidates 1 .. V-1
 * (index 0 is never drawn, seq2seq.py:1250; top_k > 0: the first min(top_k, V-1) of them in the order of casv_score_get_alternatives)
 * with weights expf((x_v - m_C) / temperature) -- x the row's logits, m_C the candidates' maximum -- by inverting the float64
 * prefix sums in ascending index order at u * Z, u = (o >> 8) * 2^-24 with o the first word of Philox4x32-10 on the counter
 * (stream[b] low word, stream[b] high word, n, s) under the key (seed low, seed high); stream NULL: stream[b] = b.  The next step's
 * decoder input is the one-hot row of v (seq2seq.py:1251), not the softmax (seq2seq.py:1252).
 * out_idx (B*samples, S) the indices; out_logp the model's log-probability of v over all V at temperature 1, in the form of
 * casv_score_targets; out_logq the proposal's, (x_v - m_C) / temperature - log Z; out_len (B*samples) = steps up to and including
 * the first end-of-line index (S if there is none; what a row produces after it is unspecified); out_align (B*samples, S, T) or
 * NULL.  A row's results are a function of (weights, line, seed, stream, n, temperature, top_k) only, whatever B, samples, the row's
 * place and the launch shape.  A row whose logits hold a NaN or whose candidates' maximum is not finite reports index 1 with NaN
 * logp / logq, feeds back an all-zero row and ends there; the call fills every output and returns CASV_ERR_NAN (the other rows
 * are untouched), like mode 1 of casv_decode_greedy.  Arithmetic: the search's (casv_decode_beam), the "arithmetic" option
 * overrides.  Always per step; with the "graph" option the steps are still launched eagerly.  Refused with CASV_ERR_ARG before
 * anything is enqueued: NULL outputs (out_align excepted), S outside 1 .. 2 * 4096, samples < 1, a temperature that is not
 * finite or <= 0, top_k outside 0 .. 64.  casv_get_alignments_sparse afterwards serves the call's B*samples rows.  Kernel class of
 * casv_profile_read: "sample". */
typedef struct {
    uint64_t seed;
    float temperature;
    int32_t top_k;
    int32_t samples;
} casv_sample_params;
int casv_decode_sample(casv_model* m, const casv_sample_params* p, int32_t S, const int64_t* stream,
                       int32_t* out_idx, float* out_logp, float* out_logq, int32_t* out_len, float* out_align);
/* Test support: the sampling kernel alone on the caller's logits (R,V), laid out as casv_debug_score_rows lays them out (pad_value
 * fills the padding columns), as step `step` of rows with stream ids stream (R; NULL: the row's number) and sample numbers sample
 * (R; NULL: 0).  u (R) non-NULL: these uniforms in place of the generator's.  out_idx / out_logp / out_logq (R); out_feedback
 * (R, Vp), Vp = V rounded up to a multiple of 32: the row the next step would read.  p->samples is ignored. */
int casv_debug_sample_rows(casv_model* m, int32_t R, int32_t V, const casv_sample_params* p, int32_t step,
                           const int64_t* stream, const int32_t* sample, const float* logits, const float* u,
                           float pad_value, int32_t* out_idx, float* out_logp, float* out_logq, float* out_feedback);
/* Sampling under a cut: the draw of casv_decode_sample from a truncated candidate set.
 * top_k in 0 .. 4095 (0 = none), top_p in (0, 1] (exactly 1 = none).  For a valid row, with the candidates 1 .. V-1, m_C and the
 * float32 weights w_v = expf((x_v - m_C) / temperature) of casv_decode_sample:
 *   a. the candidates in the order of casv_score_get_alternatives (x descending, -0 = +0, the lower index first among equals);
 *      place 0 is the maximum; top_k > 0 keeps the places j < min(top_k, V-1);
 *   b. top_p < 1: over the n places that survive (a), float64 prefix sums in place order -- lane l of 64 owns the places
 *      [l * ceil(V/64), (l+1) * ceil(V/64)) and adds their weights in ascending order, the lanes' offsets come from one sequential
 *      pass over the lanes in ascending order, P_j = off_l + run_j, Z_s = P_{n-1}; the nucleus is the places 0 .. j*, j* the first j
 *      with P_j >= (double)top_p * Z_s.  It is never empty, holds no candidate of weight 0, and a tie group at its border is entered
 *      in index order, not taken whole;
 *   c. the kept candidates are drawn from as casv_decode_sample draws: the prefix sums in ascending INDEX order inverted at u * Z,
 *      logq = (x_v - m_C) / temperature - log Z with Z the kept set's total.
 * (top_k <= 64, 1.0) gives every output bit of casv_decode_sample at that top_k; a row whose nucleus has n members gives the bits
 * of top_k = n; the smallest positive top_p gives the bits of top_k = 1.  A row's results are a function of (weights, line, seed,
 * stream, n, temperature, cut) only.  In the _cut entries p->top_k must be 0: the cut carries it.  Refused with CASV_ERR_ARG before
 * anything is enqueued or cleared: NULL cut, top_k outside 0 .. 4095, top_p NaN, <= 0 or > 1, p->top_k != 0, and whatever the
 * entry without a cut refuses.  Everything else -- CASV_ERR_NAN, the arithmetic, the eager launches, the give-up path,
 * casv_get_alignments_sparse afterwards, the kernel class "sample" -- is casv_decode_sample's.  The _cut entries always run
 * sample_cut_kernel (a wave-wide sort of the row's keys in LDS), the entries without a cut never do. */
typedef struct {
    int32_t top_k;
    float top_p;
} casv_sample_cut;
int casv_decode_sample_cut(casv_model* m, const casv_sample_params* p, const casv_sample_cut* cut, int32_t S, const int64_t* stream,
                           int32_t* out_idx, float* out_logp, float* out_logq, int32_t* out_len, float* out_align);
/* Test support: casv_debug_sample_rows under a cut.  casv_get_stat "sample_cut_rows" then reports the rows per workgroup of the
 * launch (they follow from V; the option "sample_cut_rows" bounds them). */
int casv_debug_sample_cut_rows(casv_model* m, int32_t R, int32_t V, const casv_sample_params* p, const casv_sample_cut* cut,
                               int32_t step, const int64_t* stream, const int32_t* sample, const float* logits, const float* u,
                               float pad_value, int32_t* out_idx, float* out_logp, float* out_logq, float* out_feedback);

/* The soft alignments of the LAST casv_decode_greedy / casv_decode_beam call in window form, for the post-decode
 * re-alignment of wrapper/transcode.py:126,279-349 (which skips entries <= 1/V anyway, transcode.py:316): the attention
 * of attention.py:553-571 is zero outside a window of <= 2*window_width+1 positions, so step s of result row n is
 * out_lo[n*S+s] = first position of the window (-1: the row is all NaN, the window fell off the line) and
 * out_w[(n*S+s)*K + k] = weight at position lo+k (zeros beyond the window; a rejection step of the beam is the one-hot
 * row at its source position, seq2seq.py:1495).  Rows and S as in the decode call (greedy: B rows; beam: B*max_results;
 * steps beyond a result's length are zero).  12 instead of T floats per step cross PCIe.  K >= 2*window_width+1. */
int casv_get_alignments_sparse(casv_model* m, int32_t K, int32_t* out_lo, float* out_w);

/* Host-side (no device call): the Viterbi re-alignment of wrapper/transcode.py:279-349 (`_alignment2path`) on the window form
 * of ONE line's alignments (n_rows steps: lo (n_rows) first position or -1 = all-NaN row, w (n_rows, K) weights), for the
 * first i_max input and j_max output positions, visiting cells with a score above min_score (the wrapper passes 1/voc_size,
 * transcode.py:127).  path (i_max + 1): output position of every input position on the path, -1 where the path does not pass
 * (path[i_max] = j_max, path[0] = 0, as the reference's dictionary); *dist = sum of 1 - score along the path.  Same float32
 * forward scores, tie rules and border behaviour (numpy's index -1) as the reference. */
int casv_realign_path(int32_t n_rows, int32_t T, int32_t K, const int32_t* lo, const float* w, int32_t i_max,
                      int32_t j_max, float min_score, int32_t* path, double* dist);

/* Adam(clipnorm) of seq2seq.py:496 (Keras defaults: lr 1e-3, beta 0.9/0.999, epsilon 1e-7, clipnorm 5). */
typedef struct {
    float lr, beta1, beta2, epsilon, clipnorm;
} casv_adam_params;

/* Start a training session: device master copies of the handle's weights plus zeroed Adam moments
 * (encoder_decoder_model.compile, seq2seq.py:494-497).  frozen_csv: comma-separated tensor-name prefixes whose
 * tensors are not trained (layer.trainable = False after load_transfer_weights, seq2seq.py:1206-1211) or NULL. */
int casv_train_begin(casv_model* m, const casv_adam_params* p, const char* frozen_csv);
/* One model.train_on_batch (mode 1, keras_train.py:195), model.test_on_batch (mode 0, keras_train.py:407: no
 * regulariser, no update) or loss + gradients without update (mode 2, parity tests).
 * enc_idx/enc_val: encoder input as in casv_encode, (B,T,A); dec_in / dec_out: (B,U) character indices of the
 * one-hot decoder input and target rows of vectorize_lines (seq2seq.py:1095-1106), -1 = true-zero row;
 * weights (B,U) temporal sample weights (seq2seq.py:1111-1112).  Dropout enters as explicit keep-masks already
 * scaled by 1/(1-rate), or NULL for none: mask_enc = 2W + (depth-1)*W floats (seq2seq.py:293-298; depth*2W with a deep
 * bidirectional encoder), mask_dec =
 * (depth-1)*W floats (seq2seq.py:363-367), mask_cell = (B, W+C) (LSTMCell(dropout), seq2seq.py:345).
 * loss = weighted categorical cross-entropy (+ embedding regulariser in the train phase); grad_norm = global
 * L2 norm of the gradients before clipping. */
int casv_train_step(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                    const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                    const float* weights, const float* mask_enc, const float* mask_dec, const float* mask_cell,
                    double* loss, double* grad_norm);
/* casv_train_step on soft targets: the target array dec_out (B,U) replaced by K (index, mass) slots per position, soft_idx /
 * soft_q (B,U,K), 1 <= K <= min(V, 64) -- the sparse form of the dense float y_true (B,U,V) that the reference's graph takes
 * (seq2seq.py:491-497; Keras' categorical_crossentropy is defined for any such row), and what casv_score_get_alternatives emits.
 * Slot k of a position is (i_k, q_k): i_k = -1 marks an empty slot (its q_k is ignored); a position whose slots are all empty is
 * a true-zero target row (no loss, a zero gradient row, like dec_out = -1); q_k is a finite float >= 0; the indices of one
 * position are distinct; the masses need not sum to 1.  With x the row's V logits, m, sum and p_v = expf(x_v - m) / sum as the hard
 * head forms them, w the position's weight and inv_count = 1 / max(number of nonzero weights, 1):
 *   ok_k      = 1e-7 < p[i_k] < 1 - 1e-7                       (tf.clip_by_value passes gradient inside only, per entry)
 *   loss     += w * inv_count * sum_k q_k * -logf(clip(p[i_k], 1e-7, 1 - 1e-7))
 *   S         = sum_k q_k * ok_k
 *   dlogit[v] = (p_v * S - sum_{k: i_k == v} q_k * ok_k) * w * inv_count
 * the sums over k in one fixed order (a wave butterfly over the slots) whatever the launch shape.  One slot (dec_out, 1.0) per
 * position gives casv_train_step's loss and gradients bit for bit with "deterministic".  Modes, masks, weights, the options
 * ("deterministic", "persistent", "fused_backward", the arithmetic), the give-up path and everything behind dL/dlogits are
 * casv_train_step's.  Checked on the host before anything is launched or cleared, each CASV_ERR_ARG with the session's step
 * count, moments and gradients untouched: K outside [1, min(V, 64)]; an index outside [-1, V); a mass that is negative, NaN or
 * infinite in a non-empty slot; an index repeated within a position. */
int casv_train_step_soft(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                         const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, int32_t K,
                         const int32_t* soft_idx, const float* soft_q, const float* weights, const float* mask_enc,
                         const float* mask_dec, const float* mask_cell, double* loss, double* grad_norm);
/* Test support, like casv_debug_score_rows: the soft-target loss head alone on the caller's logits (R,V), slots soft_idx / soft_q
 * (R,K) and weights (R), with the caller's inv_count; the slots are checked as casv_train_step_soft checks them.  The entry lays
 * the rows out with the row stride Vp = (V+31)&~31 and fills the columns [V, Vp) with pad_value, which no output may depend on.
 * *loss = the rows' loss (ordered != 0: summed as the "deterministic" step sums it); want_grad != 0: dlogits (R,V) = the first V
 * columns after the launch, and the entry checks that the padding columns came back as zeros (CASV_ERR_HIP with a message
 * otherwise); want_grad = 0: the logits are not written and dlogits may be NULL. */
int casv_debug_soft_ce_rows(casv_model* m, int32_t R, int32_t V, int32_t K, const float* logits, const int32_t* soft_idx,
                            const float* soft_q, const float* weight, float inv_count, float pad_value, int32_t want_grad,
                            double* loss, float* dlogits, int32_t ordered);
/* casv_train_step with the minimum-risk head (Shen et al. 2016) in place of the cross-entropy: the expected
 * cost of N costed candidates per source under the model's own distribution renormalised over the set.  Arrays, masks, the options
 * ("deterministic", "persistent", "fused_backward", the arithmetic), the give-up path, clip and Adam are casv_train_step's.  The
 * rows form G = B / N groups of N candidates, candidate i of group g being line b = g * N + i; the caller puts the same source
 * into the rows of a group (the entry does not check it, the math does not need it).  cost (B) float32: a finite value >= 0 makes
 * the line a member of its group with that cost, any negative value marks a line that is not a member (padding, or a duplicate the
 * caller removed).  alpha is finite and > 0.  Per position (b,u) with t = dec_out[b,u] >= 0 and w = weights[b,u] != 0 the entry
 * forms logp[b,u] as casv_score_targets forms it (float32, log domain, not clipped), then works in float64:
 *   s_b     = sum over u ascending of (double)(w * logp[b,u])      (float32 product, double adds)
 *   members of group g:  z_i = alpha * s_i,  M = max z_i,  e_i = exp(z_i - M),  Z = sum e_i (i ascending)
 *   q_i     = e_i / Z            risk_g = sum q_i * cost_i (i ascending)
 *   inv     = 1 / max(number of groups with at least one member, 1)
 *   c_i     = alpha * q_i * (cost_i - risk_g) * inv        non-members: q = 0, c = 0
 *   loss    = sum of inv * risk_g, added in one fixed order  (+ the embedding regulariser where casv_train_step adds it)
 *   dlogit[(u,b)][v] = (float)c_b * w * ([v == t] - p_v)   p_v = expf(x_v - m) / sum as the hard head forms it
 * -- the gradient of the loss: d risk_g / d s_i = alpha * q_i * (cost_i - risk_g) and d logp / d x_v = [v == t] - p_v, so a
 * candidate that costs more than its group expects has its characters made less likely.
 * Rows with t = -1 or w = 0 get a zero gradient row; columns [V, Vp) are never read and are written as zeros.  There is no
 * inv_count and no 1e-7 clip: this is not Keras' loss (the reference has no such head).  A group without members adds nothing and
 * is not counted (its out_risk is 0); a group whose members all have s = -inf, or that holds a NaN, gives a NaN loss, as the hard
 * step does on NaN logits.  out_q (B) and out_risk (G) are doubles and may be NULL.  The sums have one order whatever the launch
 * shape: the head is deterministic with or without the "deterministic" option.  N = 1 is legal: q = 1, c = 0, a zero gradient, the
 * loss is the mean cost.  Refused with CASV_ERR_ARG before anything is enqueued or cleared, the session's step count, moments and
 * gradients untouched: mode 0; N < 1, N > 64 or B not a multiple of N; a NULL cost; a cost that is NaN or infinite; an alpha that
 * is not finite or <= 0; whatever casv_train_step refuses. */
int casv_train_step_risk(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                         const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                         const float* weights, const float* mask_enc, const float* mask_dec, const float* mask_cell,
                         int32_t N, const float* cost, double alpha, double* out_q, double* out_risk,
                         double* loss, double* grad_norm);
/* Test support, like casv_debug_soft_ce_rows: the minimum-risk head alone on the caller's logits (G*N, U, V), targets and weights
 * (G*N, U) in the caller's order and cost (G*N), checked as casv_train_step_risk checks them (targets in [-1, V)).  The entry lays
 * the rows out as the step does (row u * B + b, stride Vp = (V+31)&~31) and fills the columns [V, Vp) with pad_value, which no
 * output may depend on.  *loss, q (G*N) doubles, coef (G*N) float32; want_grad != 0: dlogits (G*N, U, V) = the first V columns after
 * the launch, and the entry checks that the padding columns came back as zeros (CASV_ERR_HIP with a message otherwise). */
int casv_debug_risk_rows(casv_model* m, int32_t G, int32_t N, int32_t U, int32_t V, const float* logits, const int32_t* target,
                         const float* weight, const float* cost, double alpha, float pad_value, int32_t want_grad,
                         double* loss, double* q, float* coef, float* dlogits);
/* casv_train_step with scheduled sampling in its parallel form (Duckworth et al. 2019): the teacher-forced
 * forward pass, then `passes` times { logits of the current tape; a pick at every decoder position from the logits of the position
 * before it; a coin per position; the decoder again on the mixed input }, then casv_train_step's loss head, backward pass, clip and
 * update on the last pass's tape.  The encoder, u and the final / bridged states are computed once; the pick carries no gradient.
 * For decoder position (b, u), x the V logits of row (u - 1, b):
 *   coin     = (o0 >> 8) * 2^-24 < ratio, o0 .. o3 = Philox4x32-10 on the counter (step_id low, step_id high, b, u) under the key
 *              (seed low, seed high): a function of (seed, step_id, b, u) only, the same in every pass of a step
 *   eligible = u >= 1 and dec_in[b,u] >= 0
 *   pick 0   = greedy: the largest x_v over v = 1 .. V-1, the lowest index among equals, -0 == +0 (index 0 is never picked)
 *   pick 1   = the draw of casv_decode_sample at top_k = 0 and `temperature`, with the uniform (o1 >> 8) * 2^-24
 *   a row with a NaN, or whose candidates' maximum is not finite, keeps dec_in[b,u] (the step's loss is then NaN anyway)
 *   mix[b,u] = the pick where the position is eligible and the coin is true, dec_in[b,u] otherwise
 * out_dec_in (passes, B, U): slice p - 1 is the mix after pass p; the last slice is the decoder input the step trained on.  With
 * ratio 0 no pass is run -- the launches and the bits of casv_train_step -- and every slice is dec_in.  Modes 1 and 2 only
 * (validation stays teacher-forced).  Refused with CASV_ERR_ARG before anything is enqueued or cleared, the session's step count,
 * moments and gradients untouched: mode 0; NULL p or out_dec_in; ratio outside [0, 1] or NaN; passes outside 1 .. 8; pick outside
 * {0, 1}; with pick 1 a temperature that is not finite or <= 0.  Everything else is casv_train_step's.  Kernel class of
 * casv_profile_read for the mix: "sample". */
typedef struct {
    uint64_t seed, step_id;
    float ratio, temperature;
    int32_t pick;                   /* 0 greedy, 1 sample */
    int32_t passes;
} casv_sched_params;
int casv_train_step_sampled(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                            const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                            const float* weights, const float* mask_enc, const float* mask_dec, const float* mask_cell,
                            const casv_sched_params* p, int32_t* out_dec_in, double* loss, double* grad_norm);
/* Test support: the mix kernel alone on the caller's R rows, laid out as casv_debug_score_rows lays them out (pad_value fills the
 * columns [V, Vp), which no output may depend on): row r is decoder position (b[r], u[r]) with the logits row logits[r] (R,V) and
 * the gold input gold[r]; out[r] = its mix.  p->passes is ignored; the other fields are checked as casv_train_step_sampled's. */
int casv_debug_sched_rows(casv_model* m, int32_t R, int32_t V, const casv_sched_params* p, const int32_t* b, const int32_t* u,
                          const float* logits, const int32_t* gold, float pad_value, int32_t* out);
/* casv_train_step_sampled with pick 1 drawing under a cut (casv_sample_cut above: the draw of casv_decode_sample_cut at p's
 * temperature, with the uniform (o1 >> 8) * 2^-24).  The cut (0, 1.0) is casv_train_step_sampled, bit for bit.  Refused with
 * CASV_ERR_ARG before anything is enqueued or cleared, the session's state untouched: NULL cut, top_k outside 0 .. 4095, top_p NaN,
 * <= 0 or > 1, a cut other than (0, 1.0) together with pick 0, and whatever casv_train_step_sampled refuses.  A position's pick
 * stays a function of (seed, step_id, b, u, the row, the cut). */
int casv_train_step_sampled_cut(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                                const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                                const float* weights, const float* mask_enc, const float* mask_dec, const float* mask_cell,
                                const casv_sched_params* p, const casv_sample_cut* cut, int32_t* out_dec_in, double* loss,
                                double* grad_norm);
/* Test support: casv_debug_sched_rows under a cut, checked as casv_train_step_sampled_cut checks it. */
int casv_debug_sched_cut_rows(casv_model* m, int32_t R, int32_t V, const casv_sched_params* p, const casv_sample_cut* cut,
                              const int32_t* b, const int32_t* u, const float* logits, const int32_t* gold, float pad_value,
                              int32_t* out);
/* Gradient of the last step for one tensor, in Keras layout (parity tests). */
int casv_train_get_gradient(casv_model* m, const char* name, float* out, int64_t capacity);
/* Adam's optimizer state of one trained tensor in Keras layout, like casv_train_get_gradient: which = 0 the first moment m,
 * 1 the second moment v.  Valid inside a session, between steps.  A frozen tensor has no state (CASV_ERR_STATE).
 * With casv_train_get_step / casv_train_set_step (the step count of Adam's bias correction) this is everything a session
 * carries from one step to the next: a fresh session given the weights, these moments and the step continues the old one
 * (bit for bit with the "deterministic" option of casv_set_option). */
int casv_train_get_state(casv_model* m, const char* name, int32_t which, float* out, int64_t capacity);
int casv_train_set_state(casv_model* m, const char* name, int32_t which, const float* data, int64_t count);
int casv_train_get_step(casv_model* m, int64_t* step);
int casv_train_set_step(casv_model* m, int64_t step);
/* Make casv_get_weight see the current training weights (ModelCheckpoint, EarlyStopping restore; seq2seq.py:619-622). */
int casv_train_sync_weights(casv_model* m);
/* End the session: the trained weights replace the handle's weights and are repacked for inference
 * (_resync_decoder after training, seq2seq.py:645). */
int casv_train_end(casv_model* m);

/* Teacher-forced log-probabilities of given targets: the forward pass of model.test_on_batch (keras_train.py:407) on the graph
 * compiled at seq2seq.py:491-497, with the per-position quantities handed back instead of the batch's clipped cross-entropy.
 * Arrays as casv_train_step: enc_idx / enc_val (B,T,A), dec_in / dec_out (B,U), -1 = true-zero row / unscored position; the two
 * decoder arrays are independent.  An entry of dec_in or dec_out outside [-1, V) is CASV_ERR_ARG, found before anything is launched.
 * Per position (b,u) with target t = dec_out[b][u], over the V logits x of the row:
 *   logp = log softmax(x)[t], computed in the log domain in float32 and NOT clipped (0 where t = -1; -inf where x[t] = -inf);
 *   best = lowest index of the row's maximum (scored or not); rank = number of entries strictly above x[t] (-1 where t = -1);
 *   a row with a NaN entry or a maximum that is not finite gives logp = NaN, best = -1, rank = -1.
 * Per line b: nll = sum over the scored positions of -(double)logp, added in double in the order of u (the same bits whatever the
 * launch shape; NaN if a logp is), count = scored positions.  align: NULL, or (B,U,T) the attention weights the cell used at
 * every step.  No masks, no regulariser; the arithmetic, "deterministic" and "persistent" govern the forward pass exactly as
 * they govern a mode-0 casv_train_step, the give-up path included ("train_persistent_launches" / "train_give_ups" report it).
 * Inside a training session the call uses the session's current weights and changes neither step count, moments nor gradients.
 * Outside one it uses the weights of the last casv_commit_weights and needs no casv_train_begin: it keeps a forward-only state
 * (weights in the train layout, forward buffers; no gradient, no Adam moment, no backward buffer) from call to call, rebuilds it
 * when the weights are committed anew, and casv_score_release, casv_train_begin and casv_model_destroy drop it;
 * casv_train_get_step still answers CASV_ERR_STATE afterwards.  Like casv_train_step the call shares the final-state buffers
 * (hfin / cfin) with the inference session and leaves the handle without an encoded batch: casv_encode again before decoding. */
int casv_score_targets(casv_model* m, int32_t B, int32_t T, int32_t U, int32_t A,
                       const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                       float* logp, int32_t* best, int32_t* rank, double* nll, int32_t* count, float* align);
/* N candidate targets per source on ONE encoder pass (keras_train.py:407 / seq2seq.py:491-497 -- kt:407 / s2s:491-497 -- as
 * casv_score_targets, which is the N = 1 call of the same code): B sources enc_idx / enc_val (B,T,A), N targets each dec_in /
 * dec_out (B,N,U).  Decoder row r = b * N + n reads the encoder outputs, u = enc_out . U_a and the final states of source b: the
 * embedding, the encoder stack and u are computed B times, not B * N times, and the encoder's buffers are held once per source.
 * logp / best / rank (B,N,U), nll / count (B,N), align NULL or (B,N,U,T): every definition, the NaN rules, "not clipped", the
 * arithmetic, "deterministic" / "persistent" with the give-up path, the forward-only state outside a session, the behaviour inside
 * one, the sharing of hfin / cfin and "leaves the handle without an encoded batch" are casv_score_targets'.  A source with fewer
 * than N candidates pads with candidates whose dec_out row is all -1 (their dec_in may be all -1 too): logp 0, rank -1, count 0,
 * nll +0.0.  N < 1 is CASV_ERR_ARG; the [-1, V) check runs over all B*N*U entries before anything is launched.
 * casv_score_get_alignments_sparse afterwards returns the (B*N, U) rows. */
int casv_score_candidates(casv_model* m, int32_t B, int32_t N, int32_t T, int32_t U, int32_t A,
                          const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                          float* logp, int32_t* best, int32_t* rank, double* nll, int32_t* count, float* align);
/* The attention rows of the LAST casv_score_targets / casv_score_candidates call (kt:407 / s2s:491-497) in window form, same
 * conventions as casv_get_alignments_sparse: lo (B,U) first position of the window (-1: the row is all NaN), w (B,U,K) the weights
 * from there (zeros beyond the window), K >= 2*window_width+1; after casv_score_candidates B is its B*N rows.  CASV_ERR_STATE once
 * a train step or casv_score_release has run since. */
int casv_score_get_alignments_sparse(casv_model* m, int32_t K, int32_t* lo, float* w);
/* The K likeliest characters and the entropy of every position of the LAST casv_score_targets / casv_score_candidates call (kt:407
 * / s2s:491-497: the rest of the distribution whose target entry the call returned), read from the logits the call left on the
 * device.  alt_idx / alt_logp (rows,U,K), entropy (rows,U) or NULL; rows = B, or B*N after casv_score_candidates (decoder row
 * b*N + n).  Per position, over the V logits x of the row, in a total order -- x descending, compared as floats (-0.0 == +0.0),
 * ties to the lower index first -- alt_idx holds the first K entries; entries equal to -inf are ordinary members (last, in index
 * order, alt_logp -inf).  alt_logp[j] = (x[alt_idx[j]] - m) - logf(sum) with the head's m and sum: the bits of the logp that
 * casv_score_targets returns for target alt_idx[j] on the same row.  entropy = logf(sum) - (sum of expf(x - m) (x - m)) / sum in
 * float32 over the entries above -inf (an -inf entry adds 0).  A row with a NaN entry or a maximum that is not finite gives
 * alt_idx -1, alt_logp NaN, entropy NaN.  Unscored positions (dec_out = -1) are filled like any other: the distribution exists
 * whether or not a target was given.  K outside [1, min(V, 64)] is CASV_ERR_ARG, found before any launch.  State rules of
 * casv_score_get_alignments_sparse: CASV_ERR_STATE when there is no scoring call to read, and once a train step or
 * casv_score_release has run since; inside and outside a training session; the call changes nothing a later call reads and may be
 * repeated, with different K, after one scoring call. */
int casv_score_get_alternatives(casv_model* m, int32_t K, int32_t* alt_idx, float* alt_logp, float* entropy);
/* Drop the forward-only state of casv_score_targets (kt:407 / s2s:491-497); allowed when there is none. */
int casv_score_release(casv_model* m);
/* Test support, like casv_debug_activation: the scoring head (kt:407 / s2s:491-497) alone on the caller's logits (R,V) and targets
 * (R); the entry lays the rows out with the library's row stride Vp and fills the padding columns [V, Vp) with pad_value, which
 * no output may depend on.  tests/test_gpu_score.py compares the results with float64. */
int casv_debug_score_rows(casv_model* m, int32_t R, int32_t V, const float* logits, const int32_t* target, float pad_value,
                          float* logp, int32_t* best, int32_t* rank);
/* Test support, the counterpart of casv_debug_score_rows for casv_score_get_alternatives (kt:407 / s2s:491-497): its kernel alone on
 * the caller's logits (R,V), 1 <= K <= min(V, 64); alt_idx / alt_logp (R,K), entropy (R) or NULL.  The entry lays the rows out with
 * the row stride Vp = (V+31)&~31 and fills the columns [V, Vp) with pad_value, which no output may depend on.
 * tests/test_gpu_score_alternatives.py compares the results with float64 and with casv_debug_score_rows. */
int casv_debug_alternatives_rows(casv_model* m, int32_t R, int32_t V, int32_t K, const float* logits, float pad_value,
                                 int32_t* alt_idx, float* alt_logp, float* entropy);

/* The vote over N candidate lines per source: the candidate with the smallest expected edit distance to the
 * others -- the minimum-Bayes-risk pick, the medoid under Levenshtein distance.  The reference has no counterpart.  sym (B,N,L)
 * holds the candidates' symbols, arbitrary int32 values compared for equality only (the facade passes Unicode code points); len
 * (B,N) their lengths in 0 .. L, or -1 for a padding candidate (a source with fewer than N); a symbol at or beyond a candidate's
 * length influences nothing.  weight (B,N) or NULL = all 1.0.  With the candidates i, j, k of one source:
 *   D[i][j] = the unit-cost Levenshtein distance (insertion, deletion, substitution 1 each) of candidates i and j, D[i][i] = 0;
 *             -1 where i or j is padding;
 *   risk[i] = the sum over the live candidates k in ascending k of weight[k] * (double)D[i][k] (mode 0), or of
 *             weight[k] * ((double)D[i][k] / (double)max(len[i], len[k], 1)) (mode 1): float64, one rounding per operation,
 *             no fused multiply-add, starting from +0.0; +inf for a padding candidate;
 *   pick    = the live candidate of smallest risk, the lowest index among equals; -1 for a source without a live candidate.
 * out_dist (B,N,N) or NULL, out_risk (B,N), out_pick (B).  A source's results are a function of its own candidates, lengths and
 * weights only, whatever B, N, L and the other sources.  Refused with CASV_ERR_ARG before anything is enqueued: B < 1, N outside
 * 1 .. 256, L outside 0 .. 8192, mode outside 0 .. 1; NULL len, out_risk or out_pick, NULL sym where L > 0; a len outside -1 .. L;
 * a weight that is negative, NaN or infinite.  The call runs on the handle's stream in scratch of its own, which the handle owns
 * and grows on demand; it reads and changes nothing of an encode, decode, score or train session and may stand between any two
 * other calls, before the weights are committed too.  Kernel class of casv_profile_read: "consensus" (one record per call, both
 * kernels). */
int casv_consensus(casv_model* m, int32_t B, int32_t N, int32_t L, int32_t mode,
                   const int32_t* sym, const int32_t* len, const double* weight,
                   int32_t* out_dist, double* out_risk, int32_t* out_pick);

/* The confusion network voted from N candidate lines per source: every candidate aligned to one of them,
 * the pivot, then a vote per column -- the input form of the model (seq2seq.py:1020-1119: a list of chunks of (chars, p)), which the
 * reference only ever receives from an OCR engine.  sym (B,N,L), len (B,N) as for casv_consensus, L at most 2048; pivot (B) names a
 * live candidate of each source, or is -1: that source is skipped (ncol 0, where all CASV_ALIGN_NONE).  With p the pivot's lp
 * symbols, c a candidate's, D[i][j] the unit-cost Levenshtein matrix of p[:i] against c[:j]:
 *   the path  walks from (lp, len[c]) to (0, 0).  At (i, j): if i, j > 0 and D[i][j] == D[i-1][j-1] + (p[i-1] != c[j-1]), c[j-1]
 *             stands against p[i-1] and the walk goes to (i-1, j-1); else if i > 0 and D[i][j] == D[i-1][j] + 1, p[i-1] stands
 *             against a gap, on to (i-1, j); else c[j-1] is an insertion in slot i (in front of p[i], behind the last symbol for
 *             i == lp), on to (i, j-1);
 *   where[c][j] = i >= 0: symbol j stands against pivot symbol i; -1 - g: it is inserted in slot g; the pivot's own where[j] = j;
 *             CASV_ALIGN_NONE at j >= len[c] and in every position of a padding candidate;
 *   columns   ins[g] = the most symbols any live candidate inserts in slot g.  In order g = 0 .. lp: ins[g] insertion columns, then
 *             (g < lp) the column of p[g]; ncol = lp + the sum of ins.  A candidate's k-th symbol of slot g, in order of j, stands
 *             in the slot's k-th insertion column;
 *   src[col][c] = the position j that candidate c puts into the column; -1: c is live and puts a gap there; -2: c is padding;
 *   mass[col][c] = for the lowest index c of a class -- the live candidates that put a gap, or those that put equal symbols -- the
 *             sum of weight[k] over the members k in ascending order: float64 from +0.0, one rounding per addition; -1.0 for
 *             every other c, padding included;
 *   best[col] = the class representative of the largest mass, the lowest index among equals.
 * Columns at or beyond ncol hold src -2, mass -1.0, best -1.  A source's results are a function of its own candidates, lengths, pivot
 * and weights only.  casv_consensus_align fills out_where (B,N,L) and out_ncol (B) and keeps symbols, lengths, where and layout on
 * the device; casv_consensus_vote(C, weight) votes on what the last casv_consensus_align of this handle left there -- out_src
 * (B,C,N), out_mass (B,C,N), out_best (B,C), weight (B,N) or NULL = all 1.0 -- and may be called again with other weights.
 * CASV_ERR_STATE: a vote without an align to read.  Refused with CASV_ERR_ARG before anything is enqueued, nothing written and the
 * kept state untouched: B < 1, N outside 1 .. 256, L outside 0 .. 2048; a NULL argument (sym and out_where may be NULL where
 * L == 0, weight always); a len outside -1 .. L; a pivot outside -1 .. N-1 or one that names a padding candidate; C < 1 or C below
 * the largest ncol; a weight that is negative, NaN or infinite.  Both run on the handle's stream in buffers of their own and may
 * stand between any two other calls, casv_consensus included, before the weights are committed too.  The direction bits of the
 * paths live in a workspace of at most 256 MiB (one source's, where that is more): the align call takes its sources in rounds,
 * with the same results.  Kernel class of casv_profile_read: "consensus", one record per call. */
#define CASV_ALIGN_NONE INT32_MIN
int casv_consensus_align(casv_model* m, int32_t B, int32_t N, int32_t L,
                         const int32_t* sym, const int32_t* len, const int32_t* pivot,
                         int32_t* out_where, int32_t* out_ncol);
int casv_consensus_vote(casv_model* m, int32_t C, const double* weight,
                        int32_t* out_src, double* out_mass, int32_t* out_best);
/* Weighted edit costs for the vote, the confusion network and the risk.  casv_consensus_costed and
 * casv_consensus_align_costed are casv_consensus and casv_consensus_align with a cost set and, beside sym (B,N,L), key (B,N,L) or
 * NULL: per symbol a second, coarser name.  Keys are arbitrary int32 values compared for equality only; a key at or beyond a
 * candidate's length influences nothing.  For symbols x, y with keys kx, ky:
 *   c(x, y) = 0 if x == y, whatever the keys; otherwise `near` if key is not NULL and kx == ky; otherwise `sub`;
 *   an insertion or a deletion costs `gap`.
 * The matrix of p against c: D[0][j] = j * gap, D[i][0] = i * gap,
 *   D[i][j] = min(D[i-1][j] + gap, D[i][j-1] + gap, D[i-1][j-1] + c(p[i-1], c[j-1])),
 * so an empty string against one of length n gives n * gap; the costs are symmetric, and so is D.  casv_consensus_costed's D[i][j]
 * is that of candidates i and j (-1 for padding, D[i][i] = 0, as in casv_consensus); its risk is
 *   mode 0: the sum of weight[k] * (double)D[i][k];
 *   mode 1: the sum of weight[k] * ((double)D[i][k] / (double)(unit * max(len[i], len[k], 1))), the product formed in int32 and
 *           converted once -- `unit` is the caller's statement of what one full edit costs;
 * in casv_consensus's order and rounding, with its pick.  casv_consensus_align_costed's path follows casv_consensus_align's rule
 * with the costs put in: the diagonal where D[i][j] == D[i-1][j-1] + c(p[i-1], c[j-1]); else up where D[i][j] == D[i-1][j] + gap;
 * else left.  where, ins, the columns, src, mass and best keep their meaning, and a vote class is still "a gap, or equal SYMBOLS":
 * keys never pool votes.  casv_consensus_vote is unchanged and votes on what the last align of the handle left, costed or not.
 * Costs {1, 1, 1, 1} with key NULL give casv_consensus's and casv_consensus_align's results.
 *   Accepted: 1 <= gap <= 255, 0 <= near <= sub <= 255, 1 <= unit <= 255 (casv_consensus_align_costed does not read unit but
 * checks it); L at most 2048 in BOTH costed calls (a wave keeps symbol, key and DP entry of every column of the longer string in
 * LDS, 16 bytes each).  Every refusal of the plain calls applies; NULL costs, a cost outside these ranges and L beyond 2048 are
 * refused too: CASV_ERR_ARG before anything is enqueued, nothing written, the kept align state untouched.  Scratch (the keys in a
 * buffer of their own beside the symbols'), stream, the rounds under the workspace budget, "may stand between any two other
 * calls, before the weights are committed too" and the profile class "consensus" are those of the plain calls. */
typedef struct { int32_t gap, sub, near, unit; } casv_edit_costs;
int casv_consensus_costed(casv_model* m, int32_t B, int32_t N, int32_t L, int32_t mode,
                          const int32_t* sym, const int32_t* key, const int32_t* len, const double* weight,
                          const casv_edit_costs* costs, int32_t* out_dist, double* out_risk, int32_t* out_pick);
int casv_consensus_align_costed(casv_model* m, int32_t B, int32_t N, int32_t L,
                                const int32_t* sym, const int32_t* key, const int32_t* len, const int32_t* pivot,
                                const casv_edit_costs* costs, int32_t* out_where, int32_t* out_ncol);
/* Test support: the workspace budget of casv_consensus_align in bytes (0: the default), so that small calls take several rounds;
 * casv_get_stat "align_rounds" reports the rounds of the last call. */
int casv_debug_set_align_budget(casv_model* m, int64_t bytes);

/* Multi-GPU: lines are independent (seq2seq.py:113 stateful=False), so one process per GPU decodes a
 * contiguous shard of the lines with its own handle and NO data-path collective; what crosses the GPUs is one all-gather
 * of fixed-width result records per batch -- RCCL over xGMI.  The reference has no counterpart (single process,
 * wrapper/transcode.py:46).  casv_comm_unique_id: rank 0 draws the 128-byte RCCL id and hands it to the other ranks by
 * whatever channel the host program has (file, socket, MPI, torch store); casv_comm_init: every rank joins with it, on its
 * handle's device; casv_comm_all_gather: `send` (bytes_per_rank bytes, host) of every rank -> `recv` (world * bytes_per_rank
 * bytes, host, rank order), staged through device memory and gathered on the handle's stream; casv_comm_all_reduce_max: the
 * maximum of one double over the ranks (step timing; also a barrier).  RCCL is opened at the first of these calls (dlopen),
 * it is not a link dependency of the library. */
int casv_comm_unique_id(void* out128);
int casv_comm_init(casv_model* m, int32_t rank, int32_t world, const void* unique_id128);
int casv_comm_all_gather(casv_model* m, const void* send, void* recv, int64_t bytes_per_rank);
int casv_comm_all_reduce_max(casv_model* m, double* value);
int casv_comm_destroy(casv_model* m);

/* Result records packed on the device, so that the gather needs no host-side packing and no host-to-device copy: one record
 * per line = 2S+4 int32 words -- S character indices, S probabilities (bit patterns), length, score (float64, 2 words), 1 --
 * the layout of cor_asv_ann_amd/sharding.py.  casv_records_reset: a zeroed buffer of `rows` records of S steps on the handle's
 * device; casv_records_append: the best result of every line of the LAST casv_decode_beam (max_results rows per line: the
 * first) or casv_decode_greedy (mode 0) call goes to records [row_offset, row_offset + B) -- a line without a finished
 * hypothesis gets what correct_lines falls back to (its input characters, probability 1, score 0; seq2seq.py:826-836), an
 * empty padding line an empty record.  The padding decision and the fallback read the input lines on the device, so the batch
 * must have gone through casv_encode: after casv_set_encoder_outputs casv_records_append returns CASV_ERR_STATE.  A greedy
 * record's score is the sum of -log((double)p) in double over the line, divided by its length; casv_records_read: the buffer to the host; casv_records_device_ptr: its device address
 * (after the handle's stream has drained) for a host program that runs the collective itself (torch.distributed);
 * casv_comm_all_gather_records: RCCL all-gather of every rank's buffer, result (world * rows records, rank order) to the host. */
int casv_records_reset(casv_model* m, int32_t rows, int32_t S);
int casv_records_append(casv_model* m, int32_t row_offset);
int casv_records_read(casv_model* m, int32_t* out);
int casv_records_device_ptr(casv_model* m, void** ptr, int64_t* bytes);
int casv_comm_all_gather_records(casv_model* m, int32_t* recv);

/* Measurement support for bench.py: per-kernel HIP-event timing on the library's stream.
 * casv_profile(m, 1) starts recording for all kernel classes, casv_profile(m, 2) only for "lstm_gemm" (fewer
 * event records inside a timed region), casv_profile(m, 3) only for every 13th launch of it (an event pair keeps the next
 * launch from overlapping the kernel's tail, ~8 us each: level 2 costs a beamed decode 2 %, level 3 0.2 %),
 * casv_profile(m, 0) stops; casv_profile_read returns, for kernel class `name`
 * ("lstm_gemm", "lstm_gemm_small", "gemm", "attention", "softmax", "beam", "embed", "persist", "sample", "consensus"), the number of launches, their
 * summed duration (ms) and their summed algorithmic FLOPs and bytes. */
int casv_profile(casv_model* m, int32_t enable);
int casv_profile_read(casv_model* m, const char* name, int64_t* launches, double* total_ms,
                      double* flops, double* bytes);
/* Measurement aid: average duration (ms) of `iters` isolated launches of the GEMM kernel on random
 * operands; lstm=1 selects the fused LSTM-cell epilogue (N = 4*units), gather=1 a permuted row index. */
int casv_debug_gemm(casv_model* m, int32_t lstm, int32_t M, int32_t N, int32_t K, int32_t gather,
                    int32_t iters, double* ms_per_launch);
/* Test support: ONE plain contraction C (M,N) = A (M,K) . Bt (N,K)^T (+ bias (N) or NULL) on the caller's operands through the
 * launcher every GEMM of the path goes through -- with whatever tile shape ("tile") and arithmetic ("arithmetic" / "split_bf16";
 * by entry point: 0) the options select; K a multiple of 32.  flags: 1 = the launcher may split K over workgroups and 2 = over the two wave groups of a
 * workgroup (the forms the train step's contractions take: sums in another order), 4 = Bt counts as a weight (the split-bf16
 * arithmetic keeps a pre-split image of it for the call), 8 = the operands lie K-MAJOR -- A is (K,M), Bt is (K,N), C = A^T . Bt, no
 * bias: the train step's weight gradients (csrc/gemm_tn.hip; csrc/gemm_tn_split.hip under the split arithmetic where M and N are
 * multiples of 256).  tests/test_gpu_gemm.py compares the result with a float64 product. */
int casv_debug_contract(casv_model* m, int32_t flags, int32_t M, int32_t N, int32_t K, const float* A, const float* Bt,
                        const float* bias, float* C);
/* Test support: ONE weight-gradient contraction as the train step launches it (csrc/gemm_tn.hip, launch_gemm_tn_any, under the train
 * step's arithmetic): C[m][n] (+)= sum_k A[k][m] * B[k][n] for m < Mstore <= M, A [K][lda], B [K][ldb], C [Mstore][ldc] (row-major,
 * copied in and out with their strides; lda, ldb, M, N multiples of 4).  flags: 1 = accumulate into the caller's C (else C =);
 * 2 = colsum[m] += sum_k A[k][m] (in/out, Mstore entries); 4 = the ordered form of the "deterministic" option (K shares from the
 * shape, partials added in share order).  casv_get_stat then reports "tn_split" (1: the bf16x3-split kernel ran), "tn_shares" (K
 * shares launched) and "tn_nonempty_shares" (shares that hold k-tiles).  A store past row Mstore - 1 is reported as an error.
 * tests/test_gpu_gemm_tn.py compares every form with a float64 product. */
int casv_debug_contract_tn(casv_model* m, int32_t flags, int32_t M, int32_t Mstore, int32_t N, int32_t K, const float* A, int64_t lda,
                           const float* B, int64_t ldb, float* C, int64_t ldc, float* colsum);
/* Test support: the activation functions every kernel inlines (csrc/common.h: fast_tanh, fast_sigmoid, lstm_cell), on n inputs.
 * which = 0: out[i] = tanh(in[i]); 1: out[i] = sigmoid(in[i]); 2: the LSTM cell on in[5i .. 5i+4] = (z_i, z_f, z_g, z_o, c_prev)
 * -> out[2i] = c, out[2i+1] = h.  tests/test_gpu_activations.py compares them with float64. */
int casv_debug_activation(casv_model* m, int32_t which, int64_t n, const float* in, float* out);
/* Test support: ONE batch of 1..4 forward GEMM jobs on the caller's host data through the launcher every GEMM of the path goes
 * through (launch_gemm_batch), with everything of csrc/gemm_args.h that a plain contraction never uses: K segments with their own
 * koff and ld, gathered rows, step addressing, the step-0 forms, the cell state, live rows, mixed batches.  epi: 0 = plain
 * epilogue for every job, 1 = fused LSTM cell (a job with epi_plain set takes the plain epilogue inside that launch).  The options
 * "tile" and "split_bf16" select tile shape and arithmetic as for casv_debug_contract.
 *   casv_debug_rows: an input whose rows move with the step -- pool [slots][pool_rows][ld]; row m of the job is row
 *   (rows ? rows[m] : m) of slot step * step_mul + step_add; at step 0 a part with skip_first counts as zeros, one with `first`
 *   ([M][ld]) takes row m of `first` instead.  K segments: width (a multiple of 32) and koff place it in Bt's K dimension.  c_in:
 *   width = N / 4.  zinit (optional, pool = NULL: none): pool_rows = M, width = N, no rows / first / skip_first.
 *   casv_debug_out: an output [slots][M][ld] on the host (data = NULL: absent); the call returns ALL slots: the addressed one
 *   as the launch left it, every byte nothing was stored to as 0xFF.
 *   step: its value; step_by_ptr = 1: the kernels read it from a device word and the immediate step of the arguments is 0 (the
 *   job must then be valid at step 0 too).
 * Everything is checked on the host before anything is launched (CASV_ERR_ARG): every row index in [0, pool_rows), every slot the
 * step selects inside its pool, widths multiples of 32, N a multiple of 128 for LSTM jobs, koff + width <= Ktot and the widths'
 * sum <= Ktot, every ld >= its width and a multiple of 4, nact (optional; values in [0, nact_group]) one entry per line of
 * nact_group rows.  Every output has one guard row behind its last slot: a store there is CASV_ERR_STATE.  casv_get_stat then
 * reports "gemm_jobs_forms" (bit f = a launch of GemmForm f, csrc/gemm_plan.h, was part of the plan that ran) and
 * "gemm_jobs_launches" (its launches).  tests/test_gpu_lstm_gemm.py compares every form with a float64 reference. */
typedef struct casv_debug_rows {
    const float* pool;
    const int32_t* rows;
    const float* first;
    int32_t slots, pool_rows, ld, width, koff, step_mul, step_add, skip_first;
} casv_debug_rows;
typedef struct casv_debug_out {
    float* data;
    int32_t slots, ld, step_mul, step_add;
} casv_debug_out;
typedef struct casv_debug_job {
    int32_t M, N, Ktot, nseg;
    casv_debug_rows a[3], c_in, zinit;
    const float* Bt;            /* [N][Ktot]; LSTM: rows gate-interleaved [unit/32][gate i,f,c,o][unit%32] */
    const float* bias;          /* [N] or NULL */
    casv_debug_out out, c_out, gates_out, out2;
    const int32_t* nact;        /* [nact_lines] or NULL */
    int32_t nact_lines, nact_group;
    int32_t b_static;           /* Bt counts as a weight: the split arithmetic may keep a pre-split image of it for the call */
    int32_t epi_plain;
} casv_debug_job;
int casv_debug_gemm_jobs(casv_model* m, int32_t epi, int32_t count, const casv_debug_job* jobs, int32_t step, int32_t step_by_ptr);
/* The same with an accumulator input per job (csrc/gemm_args.h, acc_in; acc[j].pool = NULL: none): the job's accumulators start
 * from row (rows ? rows[m] : m) of the addressed slot of acc[j] -- width = N, no first / skip_first -- instead of from zero.  Split
 * arithmetic only (CASV_ERR_ARG under arithmetic 0, and where a job with an accumulator input would not run as 128x128 split
 * tiles); K segments may be multiples of 16 wide here.  tests/test_gpu_acc_in.py: [x | h] in one launch against x alone (no bias:
 * the raw accumulators) and then h on top of them, bit for bit. */
/* Test support: u = attention_dense(enc_out), (B,T,width) floats, as the last encoder pass behind casv_encode /
 * casv_set_encoder_outputs left it on the device; CASV_ERR_STATE if none has run yet (the pass runs for the first entry point that
 * consumes it, e.g. casv_get_encoder_outputs). */
int casv_debug_get_u(casv_model* m, float* u);
int casv_debug_gemm_jobs_acc(casv_model* m, int32_t epi, int32_t count, const casv_debug_job* jobs, const casv_debug_rows* acc,
                             int32_t step, int32_t step_by_ptr);
/* The same with the train step's launch fields per job (csrc/gemm_args.h; csrc/train.hip, plain_gemm): ksplit (-1: the launcher may
 * share K out over workgroups, whose partial sums meet in float atomics; n > 1: n shares; 0 / 1: one block per tile), kgroups (2: it
 * may share K out over the two wave groups of a workgroup as well), accumulate (C += instead of C =) and out_zeroed (the caller has
 * cleared C: the launcher adds no clear of its own).  ordered = 1 runs the launch under ordered sums, as the "deterministic" train
 * step does: no launch splits K over workgroups then.  Tile shape and arithmetic come from the options "tile" and "split_bf16" as
 * above.  The addressed slot of `out` starts, over rows < M and columns < N, as uploaded from out.data with accumulate, as zeros
 * with out_zeroed, else as 0xFF; its pad columns [N, ld), every other slot and the guard row start as 0xFF in all three cases.
 * Checked on the host before anything is launched (CASV_ERR_ARG), besides everything casv_debug_gemm_jobs checks: ksplit in
 * [-1, 64], kgroups 0 or 2, the flags 0 or 1 and not both set, a field other than 0 only on the plain-epilogue jobs of an epi = 0
 * batch, ksplit other than 0 not together with step_by_ptr.  casv_get_stat reports "gemm_jobs_shares" too: the largest grid_z of
 * the plan that ran; "gemm_jobs_launches" counts a clear of C as a launch.  tests/test_gpu_plain_sums.py holds every form the
 * planner makes of these fields (tests/plain_sum_cases.py) to float64. */
typedef struct casv_debug_sum { int32_t ksplit, kgroups, accumulate, out_zeroed; } casv_debug_sum;
int casv_debug_gemm_jobs_sum(casv_model* m, int32_t epi, int32_t count, const casv_debug_job* jobs, const casv_debug_sum* sums,
                             int32_t ordered, int32_t step, int32_t step_by_ptr);
/* Test support: ONE backward time step of 1 or 2 LSTM layers on the caller's host data, as the train step launches it where a
 * layer has no persistent backward.  form 0 = the fused launch (csrc/gemm_bwd.hip: the cell's pointwise backward inside the data
 * GEMM out = dz . Bt^T), form 1 = the two launches of the options "deterministic" and "fused_backward" off (lstm_bwd_kernel, then
 * the plain GEMM batch on a cleared output; with the option "deterministic" on, that GEMM sums in its fixed order).  Per job: dh = a * mask_a + b + c from the optional inputs a [rows][lda] (mask_a [W] or
 * NULL: ones), b [rows][ldb], c [rows][ldc] (NULL: absent; W columns of each row are read); gates [rows][4W] in the interleaved
 * order [unit / 32][gate i,f,c,o][unit % 32], cell [rows][W], c_prev [rows][ld_cprev] (NULL: zeros), dc_in [rows][W] = dL/dc of
 * the step, Bt [N][4W].  Outputs, each with ONE MORE ROW than `rows`: dz [rows + 1][4W], dc [rows + 1][W] = dL/dc of the step
 * before, out [rows + 1][ld_out].  On the device they start as 0xFF bytes but out[r][0 .. N-1], r < rows, which is zeroed as the
 * kernels' contract requires (and dc in form 1, which starts as dc_in: that kernel works in place); they come back whole, so
 * every byte nothing stored to is still 0xFF.  A store to the row behind an output or to columns N .. ld_out-1 of out is
 * CASV_ERR_STATE.  Checked on the host before anything is launched (CASV_ERR_ARG, nothing is written): form 0 / 1, 1 or 2 jobs,
 * rows in [1, 65536], N in [1, 16384], W a multiple of 32 in [32, 1024] and the same in both jobs, every ld at least its width
 * (W; ld_out: N) and a multiple of 4, no required pointer NULL, mask_a only with a.  casv_get_stat then reports
 * "bwd_step_shares" and "bwd_step_groups": the K shares of the fused launch and the unit groups of 32 per share (csrc/train_plan.h,
 * bwd_step_plan; both 0 after form 1).  tests/test_gpu_bwd_step.py compares both forms with a float64 reference. */
typedef struct casv_debug_bwd_job {
    int32_t rows, W, N;
    const float* Bt;
    const float* a; int64_t lda; const float* mask_a;
    const float* b; int64_t ldb;
    const float* c; int64_t ldc;
    const float* c_prev; int64_t ld_cprev;
    const float* gates; const float* cell; const float* dc_in;
    float* dz; float* dc; float* out; int64_t ld_out;
} casv_debug_bwd_job;
int casv_debug_bwd_step(casv_model* m, int32_t form, int32_t count, const casv_debug_bwd_job* jobs);
/* Options: "graph" = replay the decode step through a captured hipGraph (1) or launch kernels eagerly (0);
 * "persistent" = greedy decoding through the persistent decoder (all steps in ONE launch, workgroups hand rows to each
 * other through memory: small batches, where a step is too short for a launch per kernel): -1 by batch size (default:
 * up to 512 lines), 0 never, 1 always -- the results are the same bit for bit; the same option governs the train step's
 * recurrences (every pair of plain layers walks its sequence in ONE launch forward and ONE backward unless 0).  (A process started
 * with CASV_FAULT_INJECTION=1 -- the test suite -- also accepts 2 = as -1, and one workgroup of the first forward recurrence leaves
 * without handing on: the give-up path, the step is redone with per-step launches; and 3 = as 1, and one workgroup of the split
 * arithmetic's persistent encoder does the same: the pass is redone with per-step launches.  Not available otherwise.)
 * The option also governs the ENCODER pass of small batches, in either arithmetic: all layers and time steps in ONE launch
 * (csrc/persist.hip for arithmetic 0; csrc/persist_split.hip for 1 / 2, i.e. for the pass behind casv_decode_beam by default) --
 * -1: up to 512 lines in arithmetic 0, up to 256 lines in arithmetic 1 / 2 (where it measured faster than the per-step launches,
 * profiles/split_persist_encoder_timing.json), 0 never, 1 wherever the kernel fits; not for residual_connections at depth >= 3 or
 * deep_bidirectional_encoder.  Same bits as the per-step launches of the same arithmetic (tests/test_gpu_split_persistent.py);
 * "fused_backward" = 1 (default): a backward time step without a persistent form is ONE launch (cell backward inside the data
 * GEMM), 0: two;
 * "deterministic" = 0 (default) / 1: casv_train_step's results (loss, grad_norm, gradients, weights, Adam's moments; modes 0, 1
 * and 2) become a function of its inputs alone -- weights, Adam state and step count, batch arrays, masks, Adam parameters and
 * frozen set -- on a given device model and build: not of the run's timing, other work on the GPU, the device's CU count or the
 * "persistent" / "fused_backward" / CASV_ATTN_DEFER choices.  Every sum runs in a fixed order and no kernel of the step adds floats
 * atomically: the recurrences take their per-step launches, no launch splits K over workgroups except the K-major weight
 * gradients, whose shares follow from the shape and are added in share order; loss, regulariser and norm are per-workgroup
 * partial sums added by one ordered pass; the embedding gradient is summed per character in row order.  Slower than the default
 * step (profiles/);
 * "lm_predict" = 0 (default) / 1: casv_decode_beam rates its children by the decoder's context-free LM (seq2seq.py:145-149, 1487-1490;
 * see casv_decode_beam); the LM jobs take the search's arithmetic, so a line's bits are a function of (weights, line, entry point,
 * lm_predict).  The greedy decodes never use it;
 * "vendor_gemm" = 0 (default): every contraction runs in this library's own kernels; 1 = calibration: the train step's plain
 * whole-sequence contractions (input projections, their data gradients) go through hipBLASLt where it can be loaded at run time
 * (bench.py reports that time beside the own-kernel figure; inference never uses it);
 * "pin_limit_mb" (default 64) = inputs of casv_encode / results of casv_decode_greedy up to this size travel through a pinned staging
 * buffer of the handle (the call returns without waiting for its copies); larger ones are copied from / to the caller's arrays directly;
 * "eos" = vocabulary index of the end-of-line character '\n' (default 1: '' and '\n' sort first, seq2seq.py:580);
 * "tile" (process-wide; alias "skinny") = tile shape of the GEMM launches: -1 by size (default), 0 always 128x128,
 * 1 always 32x128, 2 = 64x128 wherever there is no split-K -- a measurement/test switch, the values computed are the same bit
 * for bit;
 * "arithmetic" (per handle; default -1) = which matrix instruction the handle's GEMM launches run on.  Operands, accumulators and
 * results are float32 either way.  0 = the fp32-input instruction (v_mfma_f32_32x32x2_f32): every sum is ONE k-ordered fmaf
 * chain, the arithmetic of all launches up to round 5 and of the persistent small-batch kernels.  1 / 2 = every fp32 operand value
 * is taken apart into three bf16 values (round to nearest, exact sum) and six products per term are contracted on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation (1: as 128x128 tiles, csrc/gemm.hip; 2: as 256x256 tiles where a job fills the
 * chip that way, csrc/gemm_split.hip -- the same bits from both): all 24 mantissa bits take part, measured error against float64
 * <= 1.1 x the fp32 chain's (tests/test_gpu_gemm.py), at 6/16 of the matrix-pipe time -- but another summation order, so results
 * agree with arithmetic 0 (and with the oracle, within the tolerances of tests/) to rounding, not bit for bit.
 * -1 = BY ENTRY POINT (csrc/engine.h, arithmetic_of): the decoder steps of casv_decode_beam take 2 (R = lines x hypotheses rows
 * per step: the GEMM-bound bulk of the path); casv_encode / casv_set_encoder_outputs, casv_decode_greedy, casv_decoder_step and
 * casv_train_step take 0.  The choice never looks at the batch: a line's bits are a function of (weights, line, entry point) --
 * not of the batch it is decoded in, the tile shape, the launch form (persistent or per step) or the GPU of a sharded job
 * (tests/test_gpu_arithmetic.py).  With 1 / 2 the encoder pass of a small batch has a persistent form of its own (option
 * "persistent"; csrc/persist_split.hip: the same instruction, product and tile order as the per-step launches, the same bits); the
 * persistent greedy DECODER exists in arithmetic 0 only, so under 1 / 2 the greedy decodes step kernel by kernel.
 * "split_bf16" (process-wide; default -1 = none; also CASV_SPLIT_BF16 = 0 / 1 / 2 in the environment when the library is loaded):
 * override of every handle's "arithmetic" for all launches of the decode path (tests, A/B measurements).
 * "encoder_table" (per handle; default 1; CASV_ENCODER_TABLE=0 in the environment when the handle is created sets 0): 1 = layer 1 of
 * an encoder pass that runs step by step in a split arithmetic on plain text (one alternative of weight exactly 1 per position, no
 * bridge) starts its cells from a per-character table of the accumulators of E[v] . K (csrc/encoder.hip) and contracts the recurrent
 * columns only -- the same bits; 2 = also the input terms of layers 2..D ahead: per layer ONE contraction over all B x T positions, then
 * the cells one after the other on top of its rows instead of the anti-diagonal wavefront (same bits; measured slower on c3, so not
 * the default: DESIGN.md section 4.5); 0 = never.  "beam_skip_last" (per handle; default 1; CASV_BEAM_SKIP_LAST=0 likewise): 0 = debug
 * switch, the last iteration of casv_decode_beam launches its decoder step although nothing reads its results (same results).
 * "sample_cut_rows" (per handle; default 0 = as many as fit) = 1 .. 4: at most this many rows per workgroup in sample_cut_kernel's
 * launches -- a test switch, the same results bit for bit.  "align_stamps" (per handle; default 0) = 1: a measurement aid,
 * casv_consensus_align's waves add up the shader clocks of their fill and of their walk (casv_get_stat; the same results). */
int casv_set_option(casv_model* m, const char* key, int64_t value);
/* Statistics of the last call (tests): "beam_max_new_keys" = most child hypotheses one line created in one search
 * iteration of the last casv_decode_beam; "beam_sort_capacity" = how many of them are sorted in LDS at once (more are
 * sorted in runs and merged by rank); "encoder_persistent" = 1 if the encoder pass behind the last entry point ran as ONE
 * persistent launch and was not redone per step, else 0 (0 also where the entry point reused an encoding it found);
 * "decoder_persistent" = 1 if the last casv_decode_greedy delivered the results of its ONE persistent launch (csrc/persist.hip),
 * 0 if it stepped kernel by kernel -- by the option, the shape, the back-off, or because the launch gave up and the decode was
 * redone; "decode_give_ups" = persistent launches of the decode path (encoder passes and greedy decoders) that gave up on this
 * handle so far; the figures of the last plan (csrc/persist_plan.h) -- "decoder_persist_per_cu" = workgroups per CU the runtime
 * admits for the persistent decoder at this model's staged rows, "decoder_persist_g_lstm" / "_g_att" / "_g_plain" = workgroups
 * per role (all 0 where the option, the arithmetic, the device or the depth rule the launch out), "encoder_persist_per_cu" and
 * "encoder_persist_grid" = the same figure and the workgroups of the last encoder pass that was planned (grid 0: no form);
 * "encoder_table" = 1 if the last encoder pass took layer 1's input terms from the per-character table (option "encoder_table"),
 * "encoder_ahead" = 1 if it took the upper layers' input terms ahead (value 2), "encoder_table_builds" = tables built on this handle so far (one per casv_commit_weights that was followed by such a pass);
 * "cus" = compute units of the device; "tn_split" / "tn_shares" / "tn_nonempty_shares": see casv_debug_contract_tn;
 * "gemm_jobs_forms" / "gemm_jobs_launches": see casv_debug_gemm_jobs; "gemm_jobs_shares": see casv_debug_gemm_jobs_sum; "bwd_step_shares" / "bwd_step_groups": see casv_debug_bwd_step;
 * "train_persistent_launches" = persistent recurrences (at most 16: csrc/train.hip) of the last casv_train_step that ran to its
 * end without being redone -- a step redone per step after a give-up reports 0; "train_give_ups" = steps redone after a
 * give-up on this handle so far; "sample_cut_rows" = rows per workgroup of the last sample_cut_kernel launch (0: none so far);
 * "align_rounds" = launches of consensus_align_kernel the last casv_consensus_align took under its workspace budget;
 * "align_fill_ticks" / "align_walk_ticks" = with option "align_stamps" = 1 (a measurement aid, same results) the shader clocks the
 * waves of that call spent filling their direction words and walking the paths, each summed over the waves (0 without). */
int casv_get_stat(casv_model* m, const char* key, int64_t* value);
int casv_synchronize(casv_model* m);

#ifdef __cplusplus
}
#endif
#endif
