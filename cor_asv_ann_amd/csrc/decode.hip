// Host side of the decode entry points (include/cor_asv_ann_hip.h): the decoder step (seq2seq.py:416-480) as a list of launches
// built from one view (DecodeStep), the greedy and beam decode loops (seq2seq.py:1215-1544) as sequences of phases, the sampling
// decode, and the sparse alignments of what they left on the device.  No kernel lives here: decode_kernels.hip, beam_kernels.hip, persist.hip, gemm*.hip.
#include "engine.h"

// ---- decode session ----
// Identity of the device buffers a finished decode leaves its results in (casv_get_alignments_sparse reads them later through
// raw pointers kept in last_beam): changes whenever one of them has been reallocated.
unsigned long long decode_buffers_signature(const casv_model* m) {
    unsigned long long h = 1469598103934665603ull;
    for (const DevBuf* b : {&m->st_a, &m->st_q, &m->st_win, &m->b_parent, &m->b_chr, &m->b_prob, &m->b_cum, &m->b_len, &m->b_exp, &m->b_k, &m->b_rejpos,
                            &m->b_count, &m->b_fkey, &m->b_fid, &m->b_fn, &m->b_ftotal, &m->b_created, &m->bo_idx, &m->bo_prob, &m->bo_len,
                            &m->bo_score, &m->o_idx, &m->o_prob, &m->d_idx, &m->d_val})
        h = (h ^ (unsigned long long)(uintptr_t)b->p) * 1099511628211ull;
    return h;
}

struct BufPlan { DevBuf* buf; size_t bytes; };          // (0 bytes: not needed by this call)
template <size_t K> static int ensure_all(const BufPlan (&plan)[K]) {
    for (const BufPlan& b : plan) if (int rc = b.buf->ensure(b.bytes)) return rc;
    return 0;
}

static int ensure_session(casv_model* m, int R, int S) {
    const int W = m->W, Vp = m->Vp, C = m->C, T = m->T, D = m->D;
    const size_t slots = (size_t)(S + 1) * R;
    for (int n = 1; n <= D; ++n) {
        if (int rc = m->st_h[n].ensure(slots * W * 4)) return rc;
        if (int rc = m->st_c[n].ensure(slots * W * 4)) return rc;
    }
    const BufPlan plan[] = {
        {&m->st_a, slots * T * 4}, {&m->st_p, slots * Vp * 4}, {&m->st_win, slots * 4},
        {&m->ctx, (size_t)R * C * 4}, {&m->wq, (size_t)R * W * 4}, {&m->logits, (size_t)R * Vp * 4}, {&m->prev, (size_t)R * 4},
        {&m->pin, (size_t)R * Vp * 4}, {&m->apos, (size_t)R * 8}, {&m->amax1, (size_t)R * 4}, {&m->d_step, 16}, {&m->d_nan, 16}};
    if (int rc = ensure_all(plan)) return rc;
    m->R = R; m->S = S;
    return 0;
}

static int too_many_ops() { return fail(CASV_ERR_STATE, "too many set-up operations for one launch"); }

// Initial decoder state = encoder final states (seq2seq.py:339,352), zero alignment, zero input -- and whatever else the caller
// wants cleared ahead of its first step (`ops`: result arrays, hand-off counters): ONE launch for all of it (a memset or row
// scatter of its own costs ~5 us of an otherwise idle GPU each: 13 of them in front of every batch of configs[1]).
static int init_root(casv_model* m, int rows_per_line, SmallOps ops = SmallOps{}) {
    const int W = m->W, Vp = m->Vp, T = m->T, D = m->D, R = m->R, B = m->B;
    // The operations of one launch run in no order among themselves: the initial alignment must not be both cleared and copied
    // by it.  One row per line: the copy covers the whole slot.  Several: the clear goes ahead as a launch of its own.
    bool ok = true;
    if (!m->has_a0) ok = ops.fill(m->st_a.p, (size_t)R * T * 4);
    else if (rows_per_line != 1 || R != B) HIPCHK(hipMemsetAsync(m->st_a.p, 0, (size_t)R * T * 4, m->stream));
    if (m->has_a0) ok = ok && ops.rows(m->a0.as<float>(), T, m->st_a.as<float>(), T, B, T, rows_per_line);
    ok = ok && ops.fill(m->st_p.p, (size_t)R * Vp * 4) && ops.fill(m->logits.p, (size_t)R * Vp * 4);
    for (int n = 1; n <= D; ++n) {
        ok = ok && ops.rows(m->hfin.as<float>() + (size_t)(n - 1) * B * W, W, m->st_h[n].as<float>(), W, B, W, rows_per_line);
        ok = ok && ops.rows(m->cfin.as<float>() + (size_t)(n - 1) * B * W, W, m->st_c[n].as<float>(), W, B, W, rows_per_line);
    }
    ok = ok && ops.fill(m->d_step.p, 16) && ops.fill(m->d_nan.p, 16);
    if (!ok || !launch_small_ops(ops, m->stream)) return too_many_ops();
    return 0;
}

// ---- one decoder step ----
// The view of one decoder_model step on the session's R rows (seq2seq.py:416-480): every launch of the step builds its arguments
// from (m, step) alone.
// What a sampling step draws by (casv_decode_sample)
struct SampleDraw {
    unsigned long long seed; float temperature; int top_k; const long long* stream; float* logp; float* logq;
    const casv_sample_cut* cut;     // casv_decode_sample_cut: the draw under this cut, by sample_cut_kernel (nullptr: sample_kernel at top_k)
};

struct DecodeStep {
    bool beam = false;             // input rows from `pin` and parents through `prev` (the search), otherwise row r continues row r
                                    // of the previous slot of the stores (the fed-back softmax, seq2seq.py:1252)
    bool lm = false;                // lm_predict (seq2seq.py:464-470): also the LM output, see launch_step
    bool softmax = true;            // (the beam step kernel computes the rows it reads itself)
    int mode = -1;                  // greedy pick rule of the softmax launch; -1: probabilities only
    const SampleDraw* draw = nullptr;   // the pick is a draw and the fed-back row its one-hot row (step_sample), in place of the softmax launch
    const int* line = nullptr;      // line of every row, or (nullptr) row / rows_per_line
    int rows_per_line = 1;
    int* o_idx = nullptr; float* o_prob = nullptr;          // greedy results [R][S]
    // The step number: eagerly an immediate, under graph replay read from device memory (StepRunner).
    const int* step_ptr = nullptr; int step_imm = 0;
    // Live rows per line (of `live_group` rows each), handed to the step's kernels when skipping can pay: owned by the search loop
    // (beam_search), null under graph capture, whose kernel arguments are fixed.
    const int* live = nullptr; int live_group = 0;
};

// previous-step rows of the state stores: the beam gathers its parents' expansions through `prev`; without a beam
// row r of step t simply continues row r of step t-1 (slot arithmetic, no index array and no kernel to fill one)
static const int* prev_rows(const casv_model* m, const DecodeStep& st) { return st.beam ? m->prev.as<int>() : nullptr; }
static long long slot_floats(const casv_model* m) { return (long long)m->R * m->W; }
static Seg hseg(const casv_model* m, const DecodeStep& st, float* base, int off) {
    return st.beam ? mkseg(base, m->W, m->W, off, prev_rows(m, st)) : mkseg(base, m->W, m->W, off, nullptr, slot_floats(m), 1, 0);
}
// layer input: layer 1 takes the fed-back distribution itself (embedding folded into its weights,
// pack_dec1), layer n > 1 the output of layer n-1 at this step
static int xwidth(const casv_model* m, int n) { return n == 1 ? m->Vp : m->W; }
static Seg xseg(const casv_model* m, const DecodeStep& st, int n) {
    const int Vp = m->Vp;
    if (n == 1)
        return st.beam ? mkseg(m->pin.as<float>(), Vp, Vp, 0)
                       : mkseg(m->st_p.as<float>(), Vp, Vp, 0, nullptr, (long long)m->R * Vp, 1, 0);
    return mkseg(m->st_h[n - 1].as<float>(), m->W, m->W, 0, nullptr, slot_floats(m), 1, 1);
}
// the new h_D rows of this step, ungathered: A operand of the output projection and of the query computed ahead
static Seg new_top_rows(const casv_model* m) { return mkseg(m->st_h[m->D].as<float>(), m->W, m->W, 0, nullptr, slot_floats(m), 1, 1); }
static SlotPtr state_slot(const casv_model* m, const DevBuf& store) { return mkslot(store.as<float>(), m->W, slot_floats(m), 1, 1); }

// what every launch of the step is told about the step: its number and the live rows
static void stamp(GemmArgs& g, const DecodeStep& st) {
    g.step_ptr = st.step_ptr; g.step_imm = st.step_imm;
    g.nact = st.live; g.nact_group = st.live_group;
}

// attention query of this step: h_{t-1} . W_a + b_UW (attention.py:539) -- depends only on the previous step, so it
// shares the launch of layer 1 (a job with the plain epilogue) instead of waiting behind the lower layers
// The beam search computes it AHEAD, once per expansion instead of once per child row: the query of step s + 1's rows is a
// function of their parent's h_D alone, so it rides in step s's output projection (same A operand: the new h_D rows, ungathered)
// into a store indexed like the state stores, and the attention rows fetch their parent's query through `prev` -- one launch
// less per step (the same contraction per row: the same bits).
static bool query_ahead(const DecodeStep& st) { return st.beam; }
static GemmArgs query_gemm(const casv_model* m, const DecodeStep& st) {
    const int W = m->W;
    GemmArgs g{};
    g.nseg = 1; g.a[0] = query_ahead(st) ? new_top_rows(m) : hseg(m, st, m->st_h[m->D].as<float>(), 0);
    g.Bt = m->WaT.as<float>(); g.bias = m->bUW.as<float>(); g.M = m->R; g.N = W; g.Ktot = W; g.b_static = 1;
    g.out = query_ahead(st) ? state_slot(m, m->st_q) : mkslot(m->wq.as<float>(), W);
    stamp(g, st);
    return g;
}
static GemmArgs layer_gemm(const casv_model* m, const DecodeStep& st, int n) {       // layer n < D on [x | h]
    const int W = m->W;
    GemmArgs g{};
    g.nseg = 2;
    g.a[0] = xseg(m, st, n);
    g.a[1] = hseg(m, st, m->st_h[n].as<float>(), xwidth(m, n));
    g.Bt = m->dec[n].wt.as<float>(); g.bias = m->dec[n].bias.as<float>(); g.b_static = 1;
    g.M = m->R; g.N = 4 * W; g.Ktot = xwidth(m, n) + W;
    g.out = state_slot(m, m->st_h[n]);
    g.c_in = hseg(m, st, m->st_c[n].as<float>(), 0);
    g.c_out = state_slot(m, m->st_c[n]);
    stamp(g, st);
    return g;
}
static GemmArgs top_gemm(const casv_model* m, const DecodeStep& st) {      // top cell on [x | ctx | h] (attention.py:341-342, seq2seq.py:343-349)
    const int W = m->W, C = m->C, D = m->D;
    GemmArgs g{};
    g.nseg = 3;
    g.a[0] = xseg(m, st, D);
    g.a[1] = mkseg(m->ctx.as<float>(), C, C, xwidth(m, D));
    g.a[2] = hseg(m, st, m->st_h[D].as<float>(), xwidth(m, D) + C);
    g.Bt = m->dec[D].wt.as<float>(); g.bias = m->dec[D].bias.as<float>(); g.b_static = 1;
    g.M = m->R; g.N = 4 * W; g.Ktot = xwidth(m, D) + C + W;
    g.out = state_slot(m, m->st_h[D]);
    g.c_in = hseg(m, st, m->st_c[D].as<float>(), 0);
    g.c_out = state_slot(m, m->st_c[D]);
    stamp(g, st);
    return g;
}
// the LM cell beside the top cell: [x | 0] and the same h, c (the context rows are skipped: 0 . K_ctx); its c goes to a scratch
// nothing reads
static GemmArgs lm_cell_of(const casv_model* m, const DecodeStep& st, const GemmArgs& top) {
    GemmArgs g = top;
    g.nseg = 2;
    g.a[1] = hseg(m, st, m->st_h[m->D].as<float>(), xwidth(m, m->D) + m->C);
    g.a[2] = Seg{};
    g.out = mkslot(m->lm_h.as<float>(), m->W);
    g.c_out = mkslot(m->lm_c.as<float>(), m->W);
    return g;
}
static GemmArgs projection_gemm(const casv_model* m, const DecodeStep& st) {         // tied output projection (seq2seq.py:379)
    GemmArgs g{};
    g.nseg = 1; g.a[0] = new_top_rows(m);
    g.Bt = m->E.as<float>(); g.M = m->R; g.N = m->V; g.Ktot = m->W;
    g.out = mkslot(m->logits.as<float>(), m->Vp);
    stamp(g, st);
    return g;
}
// the LM's projection (seq2seq.py:468-469): the same tied weights on h of the LM cell
static GemmArgs lm_projection_of(const casv_model* m, const GemmArgs& proj) {
    GemmArgs g = proj;
    g.a[0] = mkseg(m->lm_h.as<float>(), m->W, m->W, 0);
    g.out = mkslot(m->lm_logits.as<float>(), m->Vp);
    return g;
}

// What every launch of the attention rows shares -- the per-step launch below and the persistent decoder (persist_args) must agree
// on it for the two forms to give the same bits: encoder side, alignment and window stores, shapes; one row per line in row order.
// The per-step fields (query, parents, lines, context, step, live rows) are the caller's.
static AttnArgs attention_args(const casv_model* m) {
    const int W = m->W, C = m->C, T = m->T;
    AttnArgs a{};
    a.u = m->u.as<float>(); a.enc = m->enc_out; a.va = m->va.as<float>(); a.bv = m->bv.as<float>();
    a.a_base = m->st_a.as<float>(); a.prev = nullptr; a.line = nullptr; a.rows_per_line = 1;
    a.R = m->R; a.T = T; a.W = W; a.C = C; a.window = m->cfg.window_width;
    a.u_line = (long long)T * W; a.u_time = W; a.enc_line = (long long)T * C; a.enc_time = C;
    a.win_store = m->st_win.as<int>();
    return a;
}
static void step_attention(casv_model* m, const DecodeStep& st) {
    const int W = m->W, C = m->C, T = m->T, R = m->R;
    AttnArgs a = attention_args(m);
    a.wq = query_ahead(st) ? m->st_q.as<float>() : m->wq.as<float>(); a.wq_rows = query_ahead(st) ? prev_rows(m, st) : nullptr;
    a.prev = prev_rows(m, st); a.line = st.line; a.rows_per_line = st.rows_per_line;
    a.ctx = m->ctx.as<float>();
    a.step_ptr = st.step_ptr; a.step_imm = st.step_imm; a.apos = m->apos.as<double>(); a.amax1 = m->amax1.as<int>(); a.nrows = nullptr;
    a.win_out = nullptr;
    a.nact = st.live; a.nact_group = st.live_group;
    hipEvent_t ev{};
    const double win = 2.0 * m->cfg.window_width + 1;
    m->prof_begin(PC_ATTN, (double)R * win * (4.0 * W + 2.0 * C), 4.0 * R * (win * (W + C) + W + 2.0 * T + C), ev);
    launch_attention(a, m->stream);
    m->prof_end(PC_ATTN, ev);
}
static void step_softmax(casv_model* m, const DecodeStep& st) {
    const int R = m->R, V = m->V;
    SoftmaxArgs a{};
    a.logits = m->logits.as<float>(); a.p_base = m->st_p.as<float>(); a.R = R; a.V = V;
    a.step_ptr = st.step_ptr; a.step_imm = st.step_imm; a.mode = st.mode; a.out_idx = st.o_idx; a.out_prob = st.o_prob; a.S = m->S;
    a.nan_flag = m->d_nan.as<int>();
    a.nact = st.live; a.nact_group = st.live_group;
    hipEvent_t ev{};
    m->prof_begin(PC_SOFTMAX, 4.0 * R * V, 8.0 * R * V, ev);
    launch_softmax(a, m->stream);
    m->prof_end(PC_SOFTMAX, ev);
}
static void step_sample(casv_model* m, const DecodeStep& st) {
    const int R = m->R, V = m->V, Vp = m->Vp;
    const SampleDraw& d = *st.draw;
    SampleArgs a{};
    a.logits = m->logits.as<float>(); a.feedback = m->st_p.as<float>(); a.fb_slot = (long long)R * Vp; a.R = R; a.V = V;
    a.step_ptr = st.step_ptr; a.step_imm = st.step_imm; a.rows_per_line = st.rows_per_line; a.stream = d.stream;
    a.seed = d.seed; a.temperature = d.temperature; a.top_k = d.top_k;
    a.out_idx = st.o_idx; a.out_logp = d.logp; a.out_logq = d.logq; a.S = m->S; a.out_col = 1;
    a.nan_flag = m->d_nan.as<int>();
    hipEvent_t ev{};
    m->prof_begin(PC_SAMPLE, 4.0 * R * V, 4.0 * R * (V + Vp), ev);
    if (d.cut) {                // (casv_decode_sample_cut has asked sample_cut_ready())
        a.top_k = d.cut->top_k; a.top_p = d.cut->top_p;
        m->stat_sample_cut_rows = launch_sample_cut(a, m->sample_cut_rows_opt, m->stream);
    } else launch_sample(a, m->stream);
    m->prof_end(PC_SAMPLE, ev);
}

// One decoder_model step on R rows (seq2seq.py:416-480), as its launches in order.
// st.lm also computes the LM output: the top cell once more on the decoder's own top-layer input and states with a zero context -- a
// second job of the top cell's launch that contracts the same packed weights over the x and h segments only and leaves h in
// m->lm_h -- and its tied projection, a job of the output projection's launch, into m->lm_logits.  Rows whose LM context would be
// NaN are marked by whoever reads the logits (the beam step kernel; lm_softmax_kernel).  Without it the step launches exactly what
// it launched without the option.
static void launch_step(casv_model* m, const DecodeStep& st) {
    const int D = m->D;
    // 1. layer 1, and beside it the query where it is not computed ahead (depth 1: the query alone, the top cell is layer 1)
    if (D >= 2) {
        GemmBatch b{};
        b.g[0] = layer_gemm(m, st, 1); b.count = 1;
        if (!query_ahead(st)) { b.g[1] = query_gemm(m, st); b.g[1].epi_plain = 1; b.count = 2; }
        run_gemm_batch(m, EPI_LSTM, b);
    } else if (!query_ahead(st)) {
        GemmArgs gq = query_gemm(m, st);
        run_gemm(m, EPI_PLAIN, gq);
    }
    // 2. the attention rows need only the query: ahead of the remaining layers, which can then share one launch
    step_attention(m, st);
    // 3. layers 2 .. D-1
    for (int n = 2; n < D; ++n) { GemmArgs g = layer_gemm(m, st, n); run_gemm(m, EPI_LSTM, g); }
    // 4. the top cell, and beside it the LM cell
    GemmArgs top = top_gemm(m, st);
    if (st.lm) {
        GemmBatch b{};
        b.g[0] = top; b.g[1] = lm_cell_of(m, st, top); b.count = 2;
        run_gemm_batch(m, EPI_LSTM, b);
    } else run_gemm(m, EPI_LSTM, top);
    // 5. the output projection, and beside it the next step's query (ahead) and the LM's projection
    GemmArgs proj = projection_gemm(m, st);
    if (query_ahead(st) || st.lm) {
        GemmBatch b{};
        b.g[b.count++] = proj;
        if (query_ahead(st)) b.g[b.count++] = query_gemm(m, st);
        if (st.lm) b.g[b.count++] = lm_projection_of(m, proj);
        run_gemm_batch(m, EPI_PLAIN, b);
    } else run_gemm(m, EPI_PLAIN, proj);
    // 6. softmax and pick, or the draw
    if (st.draw) step_sample(m, st);
    else if (st.softmax) step_softmax(m, st);
}

// casv_decoder_step and (lm_probs != nullptr) casv_decoder_step_lm
static int decoder_step(casv_model* m, int32_t R, const int32_t* line, const float* p_in, const float* states_in, const float* a_in,
                        float* probs, float* states_out, float* a_out, float* lm_probs) {
    if (!m || !line || !p_in || !states_in || !a_in) return fail(CASV_ERR_ARG, "null argument");
    if (!m->encoded) return fail(CASV_ERR_STATE, "casv_encode must run first");
    if (R < 1) return fail(CASV_ERR_ARG, "R must be positive");
    for (int r = 0; r < R; ++r) if (line[r] < 0 || line[r] >= m->B) return fail(CASV_ERR_ARG, "line[%d]=%d out of range", r, line[r]);
    HIPCHK(hipSetDevice(m->device));
    if (int rc = ensure_encoded(m, arithmetic_of(m, ENTRY_CHAIN))) return rc;
    if (int rc = settle_encoder(m); rc < 0) return rc;
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_CHAIN));
    const int W = m->W, V = m->V, Vp = m->Vp, T = m->T, D = m->D;
    m->last_decode = 0;         // the step overwrites slots 0 and 1 of the stores casv_get_alignments_sparse would read
    if (int rc = ensure_session(m, R, 1)) return rc;
    if (int rc = m->d_line.ensure((size_t)R * 4)) return rc;
    HIPCHK(hipMemcpyAsync(m->d_line.p, line, (size_t)R * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemsetAsync(m->st_p.p, 0, (size_t)R * Vp * 4, m->stream));
    HIPCHK(hipMemsetAsync(m->logits.p, 0, (size_t)R * Vp * 4, m->stream));
    HIPCHK(hipMemcpy2DAsync(m->st_p.p, (size_t)Vp * 4, p_in, (size_t)V * 4, (size_t)V * 4, R, hipMemcpyHostToDevice, m->stream));
    for (int n = 1; n <= D; ++n) {
        HIPCHK(hipMemcpyAsync(m->st_h[n].p, states_in + (size_t)(2 * n - 2) * R * W, (size_t)R * W * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->st_c[n].p, states_in + (size_t)(2 * n - 1) * R * W, (size_t)R * W * 4, hipMemcpyHostToDevice, m->stream));
    }
    HIPCHK(hipMemcpyAsync(m->st_a.p, a_in, (size_t)R * T * 4, hipMemcpyHostToDevice, m->stream));
    const bool lm = lm_probs != nullptr;
    if (lm) {
        const BufPlan plan[] = {{&m->lm_h, (size_t)R * W * 4}, {&m->lm_c, (size_t)R * W * 4}, {&m->lm_logits, (size_t)R * Vp * 4}, {&m->lm_probs, (size_t)R * Vp * 4}};
        if (int rc = ensure_all(plan)) return rc;
    }
    DecodeStep st;
    st.line = m->d_line.as<int>(); st.lm = lm;
    launch_step(m, st);
    if (lm) {       // the step's query (m->wq) and window (slot 1 of the window store) give the LM's NaN rows
        LmSoftmaxArgs a{};
        a.logits = m->lm_logits.as<float>(); a.probs = m->lm_probs.as<float>(); a.wq = m->wq.as<float>();
        a.va = m->va.as<float>(); a.bv = m->bv.as<float>(); a.win = m->st_win.as<int>() + R; a.R = R; a.V = V; a.W = W;
        launch_lm_softmax(a, m->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));
    if (probs) HIPCHK(hipMemcpy2D(probs, (size_t)V * 4, m->st_p.as<float>() + (size_t)R * Vp, (size_t)Vp * 4, (size_t)V * 4, R, hipMemcpyDeviceToHost));
    if (states_out)
        for (int n = 1; n <= D; ++n) {
            HIPCHK(hipMemcpy(states_out + (size_t)(2 * n - 2) * R * W, m->st_h[n].as<float>() + (size_t)R * W, (size_t)R * W * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(states_out + (size_t)(2 * n - 1) * R * W, m->st_c[n].as<float>() + (size_t)R * W, (size_t)R * W * 4, hipMemcpyDeviceToHost));
        }
    if (a_out) HIPCHK(hipMemcpy(a_out, m->st_a.as<float>() + (size_t)R * T, (size_t)R * T * 4, hipMemcpyDeviceToHost));
    if (lm) HIPCHK(hipMemcpy2D(lm_probs, (size_t)V * 4, m->lm_probs.as<float>(), (size_t)Vp * 4, (size_t)V * 4, R, hipMemcpyDeviceToHost));
    return CASV_OK;
}

extern "C" int casv_decoder_step(casv_model* m, int32_t R, const int32_t* line, const float* p_in,
                                 const float* states_in, const float* a_in, float* probs, float* states_out,
                                 float* a_out) {
    return decoder_step(m, R, line, p_in, states_in, a_in, probs, states_out, a_out, nullptr);
}

extern "C" int casv_decoder_step_lm(casv_model* m, int32_t R, const int32_t* line, const float* p_in,
                                    const float* states_in, const float* a_in, float* probs, float* states_out,
                                    float* a_out, float* lm_probs) {
    if (!lm_probs) return fail(CASV_ERR_ARG, "null argument");
    return decoder_step(m, R, line, p_in, states_in, a_in, probs, states_out, a_out, lm_probs);
}

// Runs iterations of `body(step_ptr, step_imm)` (which launches one step).  Eagerly the host passes the step number as
// an immediate -- no kernel has to fetch it from memory first (a dependent load of a line another kernel just wrote, at
// the head of every launch) and no kernel has to advance it.  Under "graph" the iterations are replays of ONE hipGraph
// captured at the first call, whose kernels read the step from device memory and whose last node advances it.
// The body takes what it needs of its caller by reference (the search's live rows change between chunks); what it read while it was
// captured stays in the graph.
struct StepRunner {
    casv_model* m; std::string key;
    // The captured kernels hold raw pointers.  Reallocations are covered by the buffer generation; the encoder outputs switch
    // between buffers WITHOUT one (casv_encode: H1 / Ha / Hb / Hc, casv_set_encoder_outputs: Hc; an initial alignment or not),
    // so their identity is part of the key too.
    StepRunner(casv_model* m_, const std::string& key_)
        : m(m_), key(key_ + "/" + std::to_string(g_devbuf_generation) + "/" + std::to_string((unsigned long long)(uintptr_t)m_->enc_out) +
                     "/" + std::to_string((unsigned long long)(uintptr_t)m_->u.p) + "/" + std::to_string((int)m_->has_a0) +
                     "/" + std::to_string(m->gemm.arithmetic) + "." + std::to_string(gemm_split_epoch())) {}
    static void drop(casv_model* m) {
        if (m->step_exec) { (void)hipStreamSynchronize(m->stream); (void)hipGraphExecDestroy(m->step_exec); m->step_exec = nullptr; }
        if (m->step_graph) { (void)hipGraphDestroy(m->step_graph); m->step_graph = nullptr; }
        m->step_graph_key.clear();
    }
    template <class F> int run(int first, int n, const F& body) {
        if (m->use_graph && !m->prof.on) {
            if (!m->step_exec || m->step_graph_key != key) {
                drop(m);
                if (m->gemm.arithmetic >= 2) {       // (split arithmetic: the weight images are made ahead of the recording, not inside it)
                    const int W = m->W, C = m->C, D = m->D, Vp = m->Vp;
                    for (int n = 1; n <= D; ++n)
                        gemm_split_prepare(m->dec[n].wt.as<float>(), 4 * W, (n == 1 ? Vp : W) + W + (n == D && D > 1 ? C : 0) + (D == 1 ? C : 0), m->stream);
                    gemm_split_prepare(m->WaT.as<float>(), W, W, m->stream);
                }
                HIPCHK(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal));
                body(m->d_step.as<int>(), 0);
                launch_advance_step(m->d_step.as<int>(), m->stream);
                hipError_t e = hipStreamEndCapture(m->stream, &m->step_graph);        // also the way out of a failed capture
                if (e != hipSuccess) { m->step_graph = nullptr; return fail(CASV_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e)); }
                e = hipGraphInstantiate(&m->step_exec, m->step_graph, nullptr, nullptr, 0);
                if (e != hipSuccess) { m->step_exec = nullptr; drop(m); return fail(CASV_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e)); }
                m->step_graph_key = key;
            }
            for (int s = 0; s < n; ++s) HIPCHK(hipGraphLaunch(m->step_exec, m->stream));
            return 0;
        }
        for (int s = 0; s < n; ++s) body(nullptr, first + s);
        return 0;
    }
};

// ---- the greedy decode as ONE persistent launch ----
// All S greedy steps in ONE launch of the persistent decoder (persist.hip): small batches, where the per-step kernels are
// bound by launch and memory latency.  Same results bit for bit (tested), same state / alignment / window stores.

// Whether a greedy decode over B lines is the persistent launch, and that launch's figures: persist_plan.h on this model's shape, the
// device's CUs and the workgroups per CU the runtime admits for the kernel with these staged rows (not asked where the option or the
// arithmetic rule the launch out anyway).  The last plan stays readable (statistics "decoder_persist_*").
static PersistDecPlan plan_decode(casv_model* m, int B) {
    const PersistDecShape s{m->D, m->W, m->Vp, m->C};
    const int arithmetic = arithmetic_of(m, ENTRY_CHAIN);
    const int per_cu = m->persist_mode == 0 || arithmetic ? 0 : persist_decode_blocks_per_cu(persist_dec_lds_bytes(s));
    const PersistDecPlan plan = plan_persist_decode(s, B, m->ncu, per_cu, m->persist_mode, arithmetic);
    m->stat_dec_plan[0] = plan.per_cu; m->stat_dec_plan[1] = plan.g_lstm; m->stat_dec_plan[2] = plan.g_att; m->stat_dec_plan[3] = plan.g_plain;
    return plan;
}
// Whether this call is the persistent launch: its plan applies and no back-off is pending (which this question uses one call of).
static bool persist_applies(casv_model* m, int B, PersistDecPlan& plan) {
    plan = plan_decode(m, B);
    return plan.applies && !persist_backed_off(m->persist_backoff);
}
static int persist_does_not_fit(const PersistDecPlan& plan) {
    return fail(CASV_ERR_ARG, "persistent decoder: rows of %d floats do not fit the LDS", plan.kmax);
}

// The launch's arguments; its workgroups split over the three roles as planned.
static void persist_args(const casv_model* m, const PersistDecPlan& plan, int mode, int S, PersistArgs& pa) {
    const int W = m->W, Vp = m->Vp, C = m->C, T = m->T, D = m->D, R = m->R;
    pa.R = R; pa.D = D; pa.W = W; pa.V = m->V; pa.Vp = Vp; pa.C = C; pa.T = T; pa.S = S; pa.mode = mode;
    for (int n = 1; n <= D; ++n) {
        pa.layer[n - 1].w = m->dec[n].pw.as<float>(); pa.layer[n - 1].bias = m->dec[n].pbias.as<float>();
        pa.layer[n - 1].Kt = m->dec[n].kin + W;
        pa.h[n - 1] = m->st_h[n].as<float>(); pa.c[n - 1] = m->st_c[n].as<float>();
    }
    pa.wa = m->WaP.as<float>(); pa.bUW = m->bUW.as<float>(); pa.e = m->EP.as<float>();
    pa.ctx = m->p_ctx.as<float>(); pa.wq = m->p_wq.as<float>(); pa.logits = m->p_logits.as<float>();
    pa.att = attention_args(m);
    pa.out_idx = m->o_idx.as<int>(); pa.out_prob = m->o_prob.as<float>(); pa.nan_flag = m->d_nan.as<int>();
    pa.counters = m->p_counters.as<unsigned>();
    pa.lda = plan.lda;
    pa.g_lstm = plan.g_lstm; pa.g_plain = plan.g_plain; pa.g_att = plan.g_att;
}

#ifdef CASV_PERSIST_PROF
// Diagnostic build: the launch's tick sums per role, and (CASV_PERSIST_PLACEMENT) which roles shared a CU.
static DevBuf& g_persist_profbuf = *new DevBuf();     // (leaked on purpose: a static DevBuf would free into a runtime that may be gone at exit)
static int persist_prof_dump(casv_model* m, const PersistArgs& pa) {
    unsigned long long h[32];
    HIPCHK(hipMemcpyAsync(h, g_persist_profbuf.p, sizeof h, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    const char* names[4] = {"layer1 (wait stats kloop cell publish gap)", "upper  (wait - kloop cell publish gap)", "att    (wait row publish)", "plain  (wait kloop publish)"};
    if (getenv("CASV_PERSIST_PLACEMENT")) {
        const int grid = pa.g_lstm + pa.g_att + pa.g_plain;
        std::vector<unsigned long long> hw(grid);
        HIPCHK(hipMemcpy(hw.data(), g_persist_profbuf.as<unsigned long long>() + 32, (size_t)grid * 8, hipMemcpyDeviceToHost));
        std::map<unsigned, std::string> cu;
        for (int g = 0; g < grid; ++g) {
            const unsigned h = (unsigned)hw[g], xcc = (unsigned)(hw[g] >> 32) & 15;
            const unsigned key = (xcc << 16) | (((h >> 13) & 7) << 8) | (((h >> 12) & 1) << 4) | ((h >> 8) & 15);   // xcc, se, sh, cu
            cu[key] += g < pa.g_lstm ? 'L' : g < pa.g_lstm + pa.g_att ? 'A' : 'P';
        }
        std::map<std::string, int> hist;
        for (auto& kv : cu) hist[kv.second]++;
        fprintf(stderr, "persist placement (%zu CUs):", cu.size());
        for (auto& kv : hist) fprintf(stderr, " %s x%d", kv.first.c_str(), kv.second);
        fprintf(stderr, "\n");
    }
    for (int r = 0; r < 4; ++r) {
        fprintf(stderr, "persist prof %s us/step:", names[r]);
        for (int k = 0; k < 6; ++k) fprintf(stderr, " %.2f", h[r * 8 + k] * 0.01 / pa.S);
        fprintf(stderr, "\n");
    }
    return 0;
}
#endif

static int decode_greedy_persistent(casv_model* m, const PersistDecPlan& plan, int mode, int S) {
    std::lock_guard<std::mutex> lock(g_persist_mutex);
    const int W = m->W, Vp = m->Vp, C = m->C, T = m->T, D = m->D, R = m->R;
    const size_t slots = (size_t)(S + 1) * R;
    const BufPlan bufs[] = {{&m->p_ctx, slots * C * 4}, {&m->p_wq, slots * W * 4}, {&m->p_logits, slots * Vp * 4}};
    if (int rc = ensure_all(bufs)) return rc;
    if (m->p_counters.cap < plan.counter_bytes) return fail(CASV_ERR_STATE, "hand-off counters not set up");      // (cleared by the caller's set-up launch)
    PersistArgs pa{};
    persist_args(m, plan, mode, S, pa);
#ifdef CASV_PERSIST_PROF
    if (int rc = g_persist_profbuf.ensure((32 + 2048) * 8)) return rc;
    HIPCHK(hipMemsetAsync(g_persist_profbuf.p, 0, (32 + 2048) * 8, m->stream));
    pa.prof = g_persist_profbuf.as<unsigned long long>();
#endif
    hipEvent_t pev{};
    {   // executed FLOPs of the launch: every step's layer, query and logits contractions over all rows; bytes: what a step
        // must move per row (state in and out, attention window, logits) -- SURVEY.md section 8(d)'s Q_row
        double fl = 0;
        for (int n = 1; n <= D; ++n) fl += 2.0 * R * 4.0 * W * pa.layer[n - 1].Kt;
        fl += 2.0 * R * W * W + 2.0 * R * Vp * W;
        const double by = 4.0 * R * (4.0 * D * W + 11.0 * (W + C) + 2.0 * m->V + 2.0 * T);
        m->prof_begin(PC_PERSIST, fl * S, by * S, pev);
    }
    persist_order_before(m->device, m->stream);
    if (launch_persist_decode(pa, m->stream)) return persist_does_not_fit(plan);
    persist_order_after(m->device, m->stream);
    m->prof_end(PC_PERSIST, pev);
    HIPCHK(hipGetLastError());
#ifdef CASV_PERSIST_PROF
    if (int rc = persist_prof_dump(m, pa)) return rc;
#endif
    // the launch's give-up word, set aside beside the encoder's (the caller brings both to the host with the results)
    SmallOps ops{};
    ops.rows(reinterpret_cast<const float*>(persist_give_up_word(m->p_counters.as<unsigned>(), plan.counter_bytes)), 1, m->d_flags.as<float>() + 1, 1, 1, 1, 1);
    if (!launch_small_ops(ops, m->stream)) return too_many_ops();
    return 0;
}

// ---- casv_decode_greedy ----
// The view of one call: the caller's arrays and how the results come back.
struct GreedyCall {
    int mode, S;
    int32_t* out_idx; float* out_prob;
    size_t nres;                    // bytes of one result array [B][S]
    bool staged;                    // results come back through the pinned staging buffer (very large ones go straight to the caller's arrays)
    unsigned* pin_flags;            // pinned: [0] the encoder's give-up word, [1] the decoder's
    PersistDecPlan plan;            // the persistent launch of the call, if it has one
};

// results and flags come back through a pinned staging buffer: three queued copies, ONE wait for the device
// (`arrays` result arrays of nres bytes each: casv_decode_sample brings back three)
static int greedy_staging(casv_model* m, GreedyCall& c, int arrays = 2) {
    const size_t need = arrays * c.nres + 64;
    c.staged = need <= m->pin_limit;
    const size_t want = c.staged ? need : 64;
    if (m->pin_out_cap < want) {
        if (m->pin_out) { (void)hipHostFree(m->pin_out); m->pin_out = nullptr; m->pin_out_cap = 0; }
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&m->pin_out), want, hipHostMallocDefault));
        m->pin_out_cap = want;
    }
    c.pin_flags = reinterpret_cast<unsigned*>(c.staged ? m->pin_out + arrays * c.nres : m->pin_out);
    return 0;
}

// the set-up of a run, as one launch
static int greedy_begin(casv_model* m, const GreedyCall& c, bool with_counters) {
    SmallOps ops{};
    ops.fill(m->o_idx.p, c.nres); ops.fill(m->o_prob.p, c.nres);
    ops.fill(m->d_flags.as<unsigned>() + 1, 4);
    if (with_counters) {
        const size_t cbytes = c.plan.counter_bytes;
        if (int rc = m->p_counters.ensure(cbytes)) return rc;
        ops.fill(m->p_counters.p, cbytes);
    }
    return init_root(m, 1, ops);
}

// One attempt behind its set-up: run (`persistent`: as one launch), fetch, settle.  `again`: a persistent launch gave up -- of the
// decoder (`persistent` is then off for the next attempt) or of the encoder, which has been redone per step.
static int greedy_attempt(casv_model* m, const GreedyCall& c, bool& persistent, bool& again) {
    if (persistent) {
        if (int rc = decode_greedy_persistent(m, c.plan, c.mode, c.S)) return rc;
    } else {
        char key[96];
        snprintf(key, sizeof key, "greedy/%d/%d/%d/%d/%d", c.mode, m->B, m->T, c.S, m->eos);
        StepRunner runner(m, key);
        DecodeStep st;
        st.mode = c.mode; st.o_idx = m->o_idx.as<int>(); st.o_prob = m->o_prob.as<float>();
        if (int rc = runner.run(0, c.S, [&](const int* step_ptr, int step_imm) {
                DecodeStep s = st; s.step_ptr = step_ptr; s.step_imm = step_imm;
                launch_step(m, s);
            })) return rc;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c.staged ? (void*)m->pin_out : (void*)c.out_idx, m->o_idx.p, c.nres, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(c.staged ? (void*)(m->pin_out + c.nres) : (void*)c.out_prob, m->o_prob.p, c.nres, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(c.pin_flags, m->d_flags.p, 8, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    const unsigned* flags = c.pin_flags;
    // a persistent launch whose hand-off wait ran out (its workgroups were not all resident: another process running a
    // persistent kernel on this GPU) loses nothing -- the per-step kernels compute the same values; start over with them
    const bool enc_was_persistent = m->enc_check_pending;
    const int redone = settle_encoder(m, &flags[0]);
    if (redone < 0) return redone;
    const bool dec_aborted = persistent && flags[1] != 0;
    if (dec_aborted) { persist_note_abort(m->persist_backoff, "decoder"); ++m->stat_decode_give_ups; persistent = false; }     // (statistic "decode_give_ups"; the encoder's: settle_encoder)
    // the back-off is reset only by an attempt in which NO persistent launch gave up (an encoder that keeps losing residency
    // must not restart its penalty at 16 because the decoder behind it happened to run through)
    if (!redone && !dec_aborted && (persistent || enc_was_persistent)) m->persist_backoff.penalty = 0;
    again = redone || dec_aborted;
    return 0;
}

// mode 1 stops a line at its end-of-line character (seq2seq.py:1344); np.nanargmax raises only if an all-NaN row
// turns up BEFORE that (the device marks such a step with a NaN probability) -- rows keep stepping in lockstep
// after their line has ended, and what they produce there is nobody's business
// -> whether such a row turned up
static bool greedy_lengths(const casv_model* m, const GreedyCall& c, int32_t* out_len) {
    const int S = c.S;
    bool nan_before_end = false;
    for (int b = 0; b < m->B; ++b) {
        int len = S;
        if (c.mode == 1)
            for (int s = 0; s < S; ++s) {
                const float pr = c.out_prob[(size_t)b * S + s];
                if (pr != pr) { nan_before_end = true; len = s + 1; break; }
                if (c.out_idx[(size_t)b * S + s] == m->eos) { len = s + 1; break; }
            }
        if (out_len) out_len[b] = len;
    }
    return nan_before_end;
}

extern "C" int casv_decode_greedy(casv_model* m, int32_t mode, int32_t S, int32_t* out_idx, float* out_prob,
                                  int32_t* out_len, float* out_align) {
    if (!m || !out_idx || !out_prob) return fail(CASV_ERR_ARG, "null argument");
    if (!m->encoded) return fail(CASV_ERR_STATE, "casv_encode must run first");
    if (mode != 0 && mode != 1) return fail(CASV_ERR_ARG, "mode must be 0 or 1");
    if (S < 1 || S > 2 * CASV_MAX_T) return fail(CASV_ERR_ARG, "S=%d out of range 1..%d", S, 2 * CASV_MAX_T);
    HIPCHK(hipSetDevice(m->device));
    if (int rc = ensure_encoded(m, arithmetic_of(m, ENTRY_CHAIN))) return rc;
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_CHAIN));
    const int B = m->B, T = m->T;
    m->last_decode = 0;         // until this call has succeeded there is nothing to take alignments from
    GreedyCall c{};
    c.mode = mode; c.S = S; c.out_idx = out_idx; c.out_prob = out_prob; c.nres = (size_t)B * S * 4;
    if (int rc = ensure_session(m, B, S)) return rc;
    const BufPlan plan[] = {{&m->o_idx, c.nres}, {&m->o_prob, c.nres}, {&m->d_flags, 64}};
    if (int rc = ensure_all(plan)) return rc;
    if (int rc = greedy_staging(m, c)) return rc;
    m->stat_dec_persistent = 0;
    bool persistent = persist_applies(m, B, c.plan);
    for (int attempt = 0; ; ++attempt) {
        bool again = false;
        if (int rc = greedy_begin(m, c, persistent)) return rc;
        if (int rc = greedy_attempt(m, c, persistent, again)) return rc;
        if (!again) break;
        if (attempt >= 2) return fail(CASV_ERR_STATE, "persistent launches keep giving up");
    }
    m->stat_dec_persistent = persistent ? 1 : 0;       // (statistic "decoder_persistent": a launch that gave up has switched it off)
    if (c.staged) { memcpy(out_idx, m->pin_out, c.nres); memcpy(out_prob, m->pin_out + c.nres, c.nres); }
    const bool nan_before_end = greedy_lengths(m, c, out_len);
    if (out_align) {   // store_a slot s+1 row b -> (b, s, :)
        for (int s = 0; s < S; ++s)
            HIPCHK(hipMemcpy2DAsync(out_align + (size_t)s * T, (size_t)S * T * 4, m->st_a.as<float>() + (size_t)(s + 1) * B * T,
                                    (size_t)T * 4, (size_t)T * 4, B, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    if (m->prof.on) m->prof.collect();
    m->last_decode = 1; m->last_S = S; m->last_rows = B; m->last_mode = mode; m->last_signature = decode_buffers_signature(m);
    if (nan_before_end && mode == 1) return fail(CASV_ERR_NAN, "All-NaN slice encountered");
    return CASV_OK;
}

// ---- casv_decode_sample ----
// N rows per line step in lockstep from the line's root; every step ends with a draw in place of the softmax (step_sample).  Session
// buffers, result staging and the encoder's give-up handling are the greedy decode's; always the per-step form, launched eagerly
// whatever the "graph" option says (a captured graph would replay another call's seed, temperature and top_k).

static int sample_arguments(const casv_model* m, const casv_sample_params* p, int S, const void* out_idx, const void* out_logp,
                            const void* out_logq, const void* out_len) {
    if (!m || !p) return fail(CASV_ERR_ARG, "null argument");
    if (S < 1 || S > 2 * CASV_MAX_T) return fail(CASV_ERR_ARG, "S=%d out of range 1..%d", S, 2 * CASV_MAX_T);
    if (p->samples < 1) return fail(CASV_ERR_ARG, "samples=%d must be positive", p->samples);
    if (!(p->temperature > 0.f) || !(p->temperature < INFINITY)) return fail(CASV_ERR_ARG, "temperature=%g must be finite and positive", (double)p->temperature);
    if (p->top_k < 0 || p->top_k > 64) return fail(CASV_ERR_ARG, "top_k=%d out of range 0..64", p->top_k);
    if (!out_idx || !out_logp || !out_logq || !out_len) return fail(CASV_ERR_ARG, "null argument");
    return 0;
}

// the root of every row: zero input, the line's final encoder states and initial alignment under each of its N rows; cleared results
static int sample_root(casv_model* m, const GreedyCall& c, int N) {
    const int W = m->W, Vp = m->Vp, T = m->T, D = m->D, R = m->R, B = m->B;
    SmallOps ops{};
    ops.fill(m->o_idx.p, c.nres); ops.fill(m->o_prob.p, c.nres); ops.fill(m->s_logq.p, c.nres);
    ops.fill(m->d_flags.as<unsigned>() + 1, 4);
    ops.fill(m->st_p.p, (size_t)R * Vp * 4); ops.fill(m->logits.p, (size_t)R * Vp * 4);
    if (!m->has_a0) ops.fill(m->st_a.p, (size_t)R * T * 4);
    ops.fill(m->d_step.p, 16); ops.fill(m->d_nan.p, 16);
    if (!launch_small_ops(ops, m->stream)) return too_many_ops();
    for (int n = 1; n <= D; ++n) {
        launch_spread_rows(m->hfin.as<float>() + (size_t)(n - 1) * B * W, m->st_h[n].as<float>(), B, N, W, m->stream);
        launch_spread_rows(m->cfin.as<float>() + (size_t)(n - 1) * B * W, m->st_c[n].as<float>(), B, N, W, m->stream);
    }
    if (m->has_a0) launch_spread_rows(m->a0.as<float>(), m->st_a.as<float>(), B, N, T, m->stream);
    return 0;
}

// One attempt: root, S steps, fetch, settle.  `again`: the persistent encoder pass behind it had given up and has been redone per step.
static int sample_attempt(casv_model* m, const GreedyCall& c, const SampleDraw& draw, int N, float* out_logq, bool& again) {
    if (int rc = sample_root(m, c, N)) return rc;
    DecodeStep st;
    st.rows_per_line = N; st.draw = &draw; st.o_idx = m->o_idx.as<int>();
    for (int s = 0; s < c.S; ++s) { st.step_imm = s; launch_step(m, st); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c.staged ? (void*)m->pin_out : (void*)c.out_idx, m->o_idx.p, c.nres, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(c.staged ? (void*)(m->pin_out + c.nres) : (void*)c.out_prob, m->o_prob.p, c.nres, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(c.staged ? (void*)(m->pin_out + 2 * c.nres) : (void*)out_logq, m->s_logq.p, c.nres, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(c.pin_flags, m->d_flags.p, 8, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    const bool enc_was_persistent = m->enc_check_pending;
    const int redone = settle_encoder(m, &c.pin_flags[0]);
    if (redone < 0) return redone;
    if (!redone && enc_was_persistent) m->persist_backoff.penalty = 0;
    again = redone > 0;
    return 0;
}

// a row's line ends with its first end-of-line index, or at an invalid row's step (NaN logp) -> whether there was such a step
static bool sample_lengths(const casv_model* m, const GreedyCall& c, int R, int32_t* out_len) {
    bool nan_before_end = false;
    for (int r = 0; r < R; ++r) {
        int len = c.S;
        for (int s = 0; s < c.S; ++s) {
            const float lp = c.out_prob[(size_t)r * c.S + s];
            if (lp != lp) { nan_before_end = true; len = s + 1; break; }
            if (c.out_idx[(size_t)r * c.S + s] == m->eos) { len = s + 1; break; }
        }
        out_len[r] = len;
    }
    return nan_before_end;
}

// the call behind casv_decode_sample (cut == nullptr) and casv_decode_sample_cut, its arguments checked
static int decode_sample_call(casv_model* m, const casv_sample_params* p, const casv_sample_cut* cut, int32_t S, const int64_t* stream,
                              int32_t* out_idx, float* out_logp, float* out_logq, int32_t* out_len, float* out_align) {
    if (!m->encoded) return fail(CASV_ERR_STATE, "casv_encode must run first");
    const int B = m->B, T = m->T, N = p->samples;
    if ((long long)(S + 1) * B * N >= (1LL << 31)) return fail(CASV_ERR_ARG, "samples=%d: (S + 1) * lines * samples rows overflow int32 (sample fewer lines or steps per call)", N);
    const int R = B * N;
    HIPCHK(hipSetDevice(m->device));
    if (int rc = ensure_encoded(m, arithmetic_of(m, ENTRY_SEARCH))) return rc;
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_SEARCH));
    m->last_decode = 0;         // until this call has succeeded there is nothing to take alignments from
    GreedyCall c{};
    c.S = S; c.out_idx = out_idx; c.out_prob = out_logp; c.nres = (size_t)R * S * 4;
    if (int rc = ensure_session(m, R, S)) return rc;
    const BufPlan plan[] = {{&m->o_idx, c.nres}, {&m->o_prob, c.nres}, {&m->s_logq, c.nres}, {&m->d_flags, 64}, {&m->s_stream, stream ? (size_t)B * 8 : 0}};
    if (int rc = ensure_all(plan)) return rc;
    if (int rc = greedy_staging(m, c, 3)) return rc;
    if (stream) HIPCHK(hipMemcpyAsync(m->s_stream.p, stream, (size_t)B * 8, hipMemcpyHostToDevice, m->stream));
    const SampleDraw draw{p->seed, p->temperature, p->top_k, stream ? m->s_stream.as<long long>() : nullptr, m->o_prob.as<float>(), m->s_logq.as<float>(), cut};
    for (int attempt = 0; ; ++attempt) {        // (the second follows an encoder pass that gave up: there is no third, see casv_decode_beam)
        bool again = false;
        if (int rc = sample_attempt(m, c, draw, N, out_logq, again)) return rc;
        if (!again) break;
        if (attempt >= 1) return fail(CASV_ERR_STATE, "the encoder pass gave up again after it was redone per step");
    }
    if (c.staged) { memcpy(out_idx, m->pin_out, c.nres); memcpy(out_logp, m->pin_out + c.nres, c.nres); memcpy(out_logq, m->pin_out + 2 * c.nres, c.nres); }
    const bool nan_before_end = sample_lengths(m, c, R, out_len);
    if (out_align) {   // store_a slot s+1 row r -> (r, s, :)
        for (int s = 0; s < S; ++s)
            HIPCHK(hipMemcpy2DAsync(out_align + (size_t)s * T, (size_t)S * T * 4, m->st_a.as<float>() + (size_t)(s + 1) * R * T,
                                    (size_t)T * 4, (size_t)T * 4, R, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    if (m->prof.on) m->prof.collect();
    // (last_mode 2: the rows are samples, not lines -- casv_records_append refuses them)
    m->last_decode = 1; m->last_S = S; m->last_rows = R; m->last_mode = 2; m->last_signature = decode_buffers_signature(m);
    if (nan_before_end) return fail(CASV_ERR_NAN, "a sampled row's logits were NaN or without a finite candidate");
    return CASV_OK;
}

extern "C" int casv_decode_sample(casv_model* m, const casv_sample_params* p, int32_t S, const int64_t* stream, int32_t* out_idx,
                                  float* out_logp, float* out_logq, int32_t* out_len, float* out_align) {
    if (int rc = sample_arguments(m, p, S, out_idx, out_logp, out_logq, out_len)) return rc;
    return decode_sample_call(m, p, nullptr, S, stream, out_idx, out_logp, out_logq, out_len, out_align);
}

// ... under a cut (top_k, top_p): the same call with sample_cut_kernel as every step's draw
extern "C" int casv_decode_sample_cut(casv_model* m, const casv_sample_params* p, const casv_sample_cut* cut, int32_t S, const int64_t* stream,
                                      int32_t* out_idx, float* out_logp, float* out_logq, int32_t* out_len, float* out_align) {
    if (int rc = sample_arguments(m, p, S, out_idx, out_logp, out_logq, out_len)) return rc;
    if (int rc = check_sample_cut(cut)) return rc;
    if (p->top_k != 0) return fail(CASV_ERR_ARG, "top_k=%d beside a cut: the cut carries it", p->top_k);
    if (!m->encoded) return fail(CASV_ERR_STATE, "casv_encode must run first");
    HIPCHK(hipSetDevice(m->device));
    if (!sample_cut_ready()) return fail(CASV_ERR_HIP, "the runtime refused sample_cut_kernel's %d bytes of dynamic LDS", SAMPLE_CUT_LDS);
    return decode_sample_call(m, p, cut, S, stream, out_idx, out_logp, out_logq, out_len, out_align);
}

// ---- casv_decode_beam ----
// The view of one call: shapes, the search's parameters, the caller's arrays.
struct BeamCall {
    int B, T, N, R, S, MR;          // lines, positions, hypotheses per line and step, rows = B * N, steps, results per line
    int CM;                         // children per expansion: at most min(beam_width_in, V) inside the beam plus the rejection candidate beyond it
    size_t OR;                      // result rows = B * MR
    bool lm;                        // option "lm_predict" (read at every call)
    BeamParams p;
    int32_t* out_idx; float* out_prob; int32_t* out_len; double* out_score; int32_t* out_rej; float* out_align;
    int32_t* n_found; int32_t* n_steps;
};

// 1. the search's shapes and every buffer of the call
static int beam_plan_buffers(casv_model* m, const BeamCall& c, BeamState& s) {
    const size_t B = c.B, R = c.R, S = c.S, T = c.T, CM = c.CM, OR = c.OR;
    const bool wide = c.N >= 64, lm = c.lm;     // (wide beams: phase A's per-row results, beam_expand_kernel)
    if (int rc = ensure_session(m, c.R, c.S)) return rc;
    s.B = c.B; s.T = c.T; s.V = m->V; s.S = c.S; s.R = c.R;
    s.node_cap = 1 + c.S * c.N * c.CM; s.q_cap = 2 * c.T * c.N; s.f_cap = 64; s.g_cap = c.N * c.CM;
    const size_t NC = B * s.node_cap;
    const BufPlan plan[] = {
        {&m->st_q, (S + 1) * R * m->W * 4},
        {&m->b_parent, NC * 4}, {&m->b_chr, NC * 4}, {&m->b_prob, NC * 4}, {&m->b_cum, NC * 8}, {&m->b_len, NC * 4},
        {&m->b_exp, NC * 4}, {&m->b_k, NC * 4}, {&m->b_rejpos, NC * 4}, {&m->b_pos, NC * 8}, {&m->b_is1, NC * 4},
        {&m->b_count, B * 4}, {&m->b_created, (S + 1) * R * CM * 2},
        {&m->b_qkey, 2 * B * s.q_cap * 8}, {&m->b_qid, 2 * B * s.q_cap * 4}, {&m->b_qn, 2 * B * 4},
        {&m->b_fkey, B * s.f_cap * 8}, {&m->b_fid, B * s.f_cap * 4}, {&m->b_fn, B * 4}, {&m->b_ftotal, B * 4},
        {&m->b_beamnode, R * 4}, {&m->b_nact, B * 4}, {&m->b_done, B * 4},
        {&m->b_steps, B * 4}, {&m->b_active, 16},
        {&m->b_gkey, 2 * B * s.g_cap * 8}, {&m->b_gid, 2 * B * s.g_cap * 4},
        {&m->b_rowrec, wide ? R * sizeof(RowRec) : 0}, {&m->b_candidx, wide ? R * CM * 2 : 0}, {&m->b_candval, wide ? R * CM * 4 : 0},
        {&m->lm_h, lm ? R * m->W * 4 : 0}, {&m->lm_c, lm ? R * m->W * 4 : 0}, {&m->lm_logits, lm ? R * m->Vp * 4 : 0},
        {&m->b_candlm, lm && wide ? R * CM * 4 : 0},
        {&m->bo_idx, OR * S * 4}, {&m->bo_prob, OR * S * 4}, {&m->bo_len, OR * 4}, {&m->bo_score, OR * 8}, {&m->bo_rej, OR * S * 4},
        {&m->bo_found, B * 4}, {&m->bo_nsteps, B * 4},
        {&m->bo_align, c.out_align ? OR * S * T * 4 : 0}};
    return ensure_all(plan);
}

// 2. the search state's pointers
static void beam_bind(const casv_model* m, const BeamCall& c, BeamState& s) {
    s.n_parent = m->b_parent.as<int>(); s.n_chr = m->b_chr.as<int>(); s.n_prob = m->b_prob.as<float>();
    s.n_cum = m->b_cum.as<double>(); s.n_len = m->b_len.as<int>(); s.n_exp = m->b_exp.as<int>(); s.n_k = m->b_k.as<int>();
    s.n_rejpos = m->b_rejpos.as<int>(); s.n_pos = m->b_pos.as<double>(); s.n_is1 = m->b_is1.as<int>();
    s.n_count = m->b_count.as<int>(); s.created = m->b_created.as<short>();
    s.q_key = m->b_qkey.as<double>(); s.q_id = m->b_qid.as<int>(); s.q_n = m->b_qn.as<int>();
    s.g_key = m->b_gkey.as<double>(); s.g_id = m->b_gid.as<int>();
    s.f_key = m->b_fkey.as<double>(); s.f_id = m->b_fid.as<int>(); s.f_n = m->b_fn.as<int>(); s.f_total = m->b_ftotal.as<int>();
    s.beam_node = m->b_beamnode.as<int>(); s.nact = m->b_nact.as<int>();
    s.line_done = m->b_done.as<int>(); s.line_steps = m->b_steps.as<int>(); s.active_lines = m->b_active.as<int>();
    s.prev = m->prev.as<int>(); s.p_in = m->pin.as<float>(); s.p_base = m->st_p.as<float>();
    s.apos = m->apos.as<double>(); s.amax1 = m->amax1.as<int>(); s.src_rej = m->d_srcrej.as<int>();
    s.step_ptr = m->d_step.as<int>();
    if (c.N >= 64) { s.rowrec = m->b_rowrec.as<RowRec>(); s.cand_idx = m->b_candidx.as<short>(); s.cand_val = m->b_candval.as<float>(); }
    if (c.lm) {
        s.lm_q = m->st_q.as<float>(); s.lm_va = m->va.as<float>(); s.lm_bv = m->bv.as<float>(); s.lm_win = m->st_win.as<int>(); s.W = m->W;
        if (c.N >= 64) s.cand_lm = m->b_candlm.as<float>();
    }
}

// 3. the root of every line: initial state, the root expansions' query, the search state
static int beam_root(casv_model* m, const BeamCall& c, const BeamState& s) {
    if (int rc = init_root(m, c.N)) return rc;
    // the root expansions' attention query (slot 0: the encoder's final h_D), as every later step's output projection leaves it
    const int W = m->W;
    GemmArgs gq{};
    gq.nseg = 1; gq.a[0] = mkseg(m->st_h[m->D].as<float>(), W, W, 0);
    gq.Bt = m->WaT.as<float>(); gq.bias = m->bUW.as<float>(); gq.M = c.R; gq.N = W; gq.Ktot = W; gq.b_static = 1;
    gq.out = mkslot(m->st_q.as<float>(), W);
    run_gemm(m, EPI_PLAIN, gq);
    launch_beam_init(s, c.p, m->stream);
    return 0;
}

// The persistent encoder's give-up word travels with the first count (beam_search).  Looked at once, behind a wait that covers its
// copy.  A pass that gave up is redone per step (settle_encoder) and the search starts over on its outputs (`redo`): nothing
// decoded from the abandoned pass is trusted.
static int beam_settle_encoder(casv_model* m, bool& enc_settled, bool& redo) {
    if (enc_settled) return 0;
    const unsigned flag = (unsigned)m->pin_active[2];
    const int redone = settle_encoder(m, &flag);
    if (redone == 0) m->persist_backoff.penalty = 0;
    enc_settled = true;
    redo = redone > 0;
    return redone < 0 ? redone : 0;
}

// 4. the search: steps in chunks, until no line is unfinished or S steps have run
static int beam_search(casv_model* m, const BeamCall& c, const BeamState& s, bool& enc_settled, bool& redo) {
    const int B = c.B, S = c.S, N = c.N;
    const BeamParams& p = c.p;
    // Tiles / rows without a live hypothesis are skipped by the step's kernels (their state is never read).  Worth the
    // extra load per workgroup from the start when a line's N rows span whole tiles (beams fill up over the first
    // steps), otherwise once a line has finished; not under graph replay, whose kernel arguments are fixed at capture.
    const int* live = (N >= 128 && !m->use_graph) ? m->b_nact.as<int>() : nullptr;
    auto body = [&](const int* step_ptr, int step_imm) {
        DecodeStep st;
        st.beam = true; st.lm = c.lm; st.softmax = false; st.rows_per_line = N;
        st.step_ptr = step_ptr; st.step_imm = step_imm; st.live = live; st.live_group = N;
        // Iteration S - 1 creates no node: the beam kernels leave at step + 1 >= S before they read a logit (beam_kernels.hip: the
        // step kernel only records line_steps, s2s:1398).  What its decoder step would write -- slot S of the state, query,
        // alignment and window stores, the logits -- is read by nobody: the extraction kernels, casv_get_alignments_sparse and the
        // records follow n_exp of nodes created at iterations <= S - 2 (slots <= S - 1), the LM jobs feed the same beam kernel.  So
        // the eager path (the step number is an immediate) launches the beam step alone; a captured body stays whole.
        // (option "beam_skip_last" = 0: the step is launched all the same -- tests compare the two)
        const bool unread = !step_ptr && step_imm == S - 1 && m->beam_skip_last;
        if (!unread) launch_step(m, st);
        hipEvent_t ev{};
        m->prof_begin(PC_BEAM, 0.0, 4.0 * c.R * ((c.lm ? 3.0 : 2.0) * m->Vp), ev);
        BeamState sb = s;
        sb.step_ptr = step_ptr; sb.step_imm = step_imm; sb.logits = m->logits.as<float>();
        if (c.lm) sb.lm_logits = m->lm_logits.as<float>();
        launch_beam_step(sb, p, m->stream);
        m->prof_end(PC_BEAM, ev);
    };
    // The host looks at the number of unfinished lines every `chunk` iterations -- one chunk behind: the count of chunk k
    // travels to pinned host memory while chunk k+1 is already queued, so the GPU never waits for the host (a blocking poll
    // cost 150 us of idle GPU every 16 steps).  A search that ends early runs at most one chunk of empty iterations.
    const int chunk = 16;
    char key[256];
    snprintf(key, sizeof key, "beam/%d/%d/%d/%d/%d/%d/%d/%.17g/%.17g/%.17g/%d%s", B, c.T, S, N, p.width_in, p.width_out, c.MR, p.threshold_in,
             p.rejection, p.cost0, p.eos, c.lm ? "/lm" : "");
    StepRunner runner(m, key);
    if (!m->pin_active) {
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&m->pin_active), 3 * sizeof(int), hipHostMallocDefault));      // ([2]: the encoder's give-up word)
        for (int k = 0; k < 2; ++k) HIPCHK(hipEventCreateWithFlags(&m->ev_active[k], hipEventDisableTiming));
    }
    enc_settled = !m->enc_check_pending;
    if (!enc_settled) HIPCHK(hipMemcpyAsync(&m->pin_active[2], m->d_flags.p, 4, hipMemcpyDeviceToHost, m->stream));
    int pending = -1;                       // slot whose copy is in flight
    int slot = 0;
    for (int done_steps = 0; done_steps < S; ) {
        const int n = (S - done_steps) < chunk ? (S - done_steps) : chunk;
        if (int rc = runner.run(done_steps, n, body)) return rc;
        done_steps += n;
        HIPCHK(hipMemcpyAsync(&m->pin_active[slot], m->b_active.p, 4, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipEventRecord(m->ev_active[slot], m->stream));
        if (pending >= 0) {                 // the chunk before this one
            HIPCHK(hipEventSynchronize(m->ev_active[pending]));
            if (int rc = beam_settle_encoder(m, enc_settled, redo)) return rc;
            if (redo) return 0;
            const int active = m->pin_active[pending];
            if (active <= 0) break;
            if (active < B && !m->use_graph) live = m->b_nact.as<int>();
        }
        pending = slot; slot ^= 1;
    }
    return 0;
}

// 5. the results: best hypotheses of every line into the result arrays, and those to the caller; one wait
static int beam_extract_fetch(casv_model* m, const BeamCall& c, const BeamState& s) {
    const size_t B = c.B, S = c.S, T = c.T, OR = c.OR;
    BeamOut o{};
    o.idx = m->bo_idx.as<int>(); o.prob = m->bo_prob.as<float>(); o.len = m->bo_len.as<int>(); o.score = m->bo_score.as<double>();
    o.rejpos = m->bo_rej.as<int>(); o.align = c.out_align ? m->bo_align.as<float>() : nullptr; o.n_found = m->bo_found.as<int>();
    o.n_steps = m->bo_nsteps.as<int>(); o.a_base = m->st_a.as<float>();
    SmallOps ops{};
    ops.fill(m->bo_idx.p, OR * S * 4); ops.fill(m->bo_prob.p, OR * S * 4); ops.fill(m->bo_rej.p, OR * S * 4, 0xffffffffu);
    if (!launch_small_ops(ops, m->stream)) return too_many_ops();
#ifdef CASV_BEAM_PROF
    { HIPCHK(hipStreamSynchronize(m->stream)); casv::beam_prof_dump(m->S); }
#endif
#ifdef CASV_GEMM_PROF
    { HIPCHK(hipStreamSynchronize(m->stream)); casv::gemm_prof_dump(); casv::skinny_prof_dump(); }
#endif
    launch_beam_extract(s, c.p, o, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c.out_idx, o.idx, OR * S * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(c.out_prob, o.prob, OR * S * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(c.out_len, o.len, OR * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(c.out_score, o.score, OR * 8, hipMemcpyDeviceToHost, m->stream));
    if (c.out_rej) HIPCHK(hipMemcpyAsync(c.out_rej, o.rejpos, OR * S * 4, hipMemcpyDeviceToHost, m->stream));
    if (c.out_align) HIPCHK(hipMemcpyAsync(c.out_align, o.align, OR * S * T * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(c.n_found, o.n_found, B * 4, hipMemcpyDeviceToHost, m->stream));
    if (c.n_steps) HIPCHK(hipMemcpyAsync(c.n_steps, o.n_steps, B * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(m->stat_beam, m->b_active.as<int>() + 1, 12, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

// One attempt of the call.  `redo`: the encoder pass behind it had given up and has been redone per step; nothing of this attempt
// counts.
static int beam_attempt(casv_model* m, const BeamCall& c, bool& redo) {
    BeamState s{};
    bool enc_settled = true;
    m->last_decode = 0;         // until this call has succeeded there is nothing to take alignments from
    if (int rc = beam_plan_buffers(m, c, s)) return rc;
    beam_bind(m, c, s);
    if (int rc = beam_root(m, c, s)) return rc;
    if (int rc = beam_search(m, c, s, enc_settled, redo)) return rc;
    if (redo) return 0;
    if (int rc = beam_extract_fetch(m, c, s)) return rc;
    if (int rc = beam_settle_encoder(m, enc_settled, redo)) return rc;      // (a search of at most two chunks: no count was waited for)
    if (redo) return 0;
    if (m->prof.on) m->prof.collect();
    m->last_decode = 2; m->last_S = c.S; m->last_rows = (int)c.OR; m->last_beam = s; m->last_beam_params = c.p;
    m->last_signature = decode_buffers_signature(m);
    return 0;
}

extern "C" int casv_decode_beam(casv_model* m, const casv_beam_params* bp, int32_t S, int32_t* out_idx, float* out_prob,
                                int32_t* out_len, double* out_score, int32_t* out_rej, float* out_align,
                                int32_t* n_found, int32_t* n_steps) {
    if (!m || !bp || !out_idx || !out_prob || !out_len || !out_score || !n_found) return fail(CASV_ERR_ARG, "null argument");
    if (!m->encoded) return fail(CASV_ERR_STATE, "casv_encode must run first");
    const int N = bp->batch_size;
    if (N < 1 || N > CASV_MAX_BEAM_N) return fail(CASV_ERR_ARG, "batch_size (hypotheses per step) %d out of range 1..%d", N, CASV_MAX_BEAM_N);
    if (bp->beam_width_in < 1) return fail(CASV_ERR_ARG, "beam_width_in %d must be positive", bp->beam_width_in);
    const int CM = (bp->beam_width_in < m->V ? bp->beam_width_in : m->V) + 1;
    if (bp->max_results < 1 || bp->max_results > 64) return fail(CASV_ERR_ARG, "max_results out of range 1..64");
    if (S < 1 || S > 2 * CASV_MAX_T) return fail(CASV_ERR_ARG, "S=%d out of range 1..%d", S, 2 * CASV_MAX_T);
    if (1LL + (long long)S * N * CM >= (1LL << 31) || (long long)(S + 1) * m->B * N >= (1LL << 31))
        return fail(CASV_ERR_ARG, "search too large: S * batch_size * (beam_width_in + 1) nodes per line overflow int32 (decode fewer lines or steps per call)");
    HIPCHK(hipSetDevice(m->device));
    if (int rc = ensure_encoded(m, arithmetic_of(m, ENTRY_SEARCH))) return rc;
    // (a persistent encoder launch's give-up word is looked at in the search, where this call first waits for the device anyway)
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_SEARCH));         // the search: bf16x3-split operands by default (engine.h)
    BeamCall c{};
    c.B = m->B; c.T = m->T; c.N = N; c.R = m->B * N; c.S = S; c.MR = bp->max_results; c.CM = CM;
    c.OR = (size_t)m->B * c.MR; c.lm = m->lm_predict;
    c.p.N = N; c.p.width_in = bp->beam_width_in; c.p.width_out = bp->beam_width_out; c.p.max_results = c.MR;
    c.p.threshold_in = bp->beam_threshold_in; c.p.rejection = bp->rejection_threshold; c.p.cost0 = bp->cost0; c.p.eos = m->eos;
    c.out_idx = out_idx; c.out_prob = out_prob; c.out_len = out_len; c.out_score = out_score; c.out_rej = out_rej; c.out_align = out_align;
    c.n_found = n_found; c.n_steps = n_steps;
    // At most two attempts: the second follows an encoder pass that gave up and was redone per step -- settle_encoder has cleared
    // enc_check_pending by then, so it cannot ask for a third.
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool redo = false;
        if (int rc = beam_attempt(m, c, redo)) return rc;
        if (!redo) return CASV_OK;
    }
    return fail(CASV_ERR_STATE, "the encoder pass gave up again after it was redone per step");
}

extern "C" int casv_get_alignments_sparse(casv_model* m, int32_t K, int32_t* out_lo, float* out_w) {
    if (!m || !out_lo || !out_w) return fail(CASV_ERR_ARG, "null argument");
    if (!m->last_decode) return fail(CASV_ERR_STATE, "no decode call to take alignments from");
    // last_beam holds raw pointers into the handle's buffers: refuse once any of them may have moved
    if (m->last_signature != decode_buffers_signature(m)) { m->last_decode = 0; return fail(CASV_ERR_STATE, "the decode results have been released (a later call reallocated device buffers)"); }
    if (K < 2 * m->cfg.window_width + 1 || K > 64) return fail(CASV_ERR_ARG, "K=%d: need at least 2*window_width+1 = %d weights per step (at most 64)", K, 2 * m->cfg.window_width + 1);
    HIPCHK(hipSetDevice(m->device));
    const size_t n = (size_t)m->last_rows * m->last_S;
    if (int rc = m->sp_lo.ensure(n * 4)) return rc;
    if (int rc = m->sp_w.ensure(n * K * 4)) return rc;
    SparseAlignOut sp{m->sp_lo.as<int>(), m->sp_w.as<float>(), K, m->st_win.as<int>()};
    if (m->last_decode == 1) {
        launch_greedy_extract_sparse(m->st_a.as<float>(), m->st_win.as<int>(), m->last_rows, m->last_S, m->T, sp, m->stream);
    } else {
        HIPCHK(hipMemsetAsync(sp.lo, 0, n * 4, m->stream));
        HIPCHK(hipMemsetAsync(sp.w, 0, n * K * 4, m->stream));
        BeamOut o{};
        o.a_base = m->st_a.as<float>();
        launch_beam_extract_sparse(m->last_beam, m->last_beam_params, o, sp, m->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_lo, sp.lo, n * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_w, sp.w, n * K * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}
