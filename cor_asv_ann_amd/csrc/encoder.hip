// The encoder pass of the C ABI (seq2seq.py:237-314): casv_encode stages a batch's inputs, run_encoder computes the outputs for the
// first entry point that needs them (ensure_encoded) in ONE of four launch forms -- persistent, wavefront, residual or deep -- and
// settle_encoder looks at a persistent launch's give-up word where the host waits for the device anyway.
#include "engine.h"

// ---- the persistent forms: the whole recurrence as ONE launch (same values bit for bit as the per-step launches) ----
// persist.hip on the fp32-input chain (tiles of 16 rows x 16 units, weights packed for it, staged rows of `lda` floats in LDS);
// persist_split.hip in the split arithmetic (tiles of 32 rows x 32 units, the per-step launches' own weights, a fixed LDS size).
// Whether a pass over B lines has a persistent form, and that form's launch -- planned once, for the decision and the launch alike:
// persist_plan.h on this model's shape, the device's CUs and the workgroups per CU the runtime admits for the form's kernel (not
// asked where the option rules the launch out anyway).  The last plan stays readable (statistics "encoder_persist_*").
static PersistEncPlan plan_persist_enc(casv_model* m, int B) {
    const PersistEncShape s{m->D, m->W, m->cfg.residual_connections != 0, m->cfg.deep_bidirectional_encoder != 0};
    const bool split = m->enc_arith > 0;
    const int per_cu = m->persist_mode == 0 ? 0
                     : split ? persist_split_encode_blocks_per_cu()
                             : persist_encode_blocks_per_cu(persist_enc_lds_bytes(s));      // 0: the staged rows do not fit the LDS
    const PersistEncPlan plan = plan_persist_encode(s, B, m->ncu, per_cu, m->persist_mode, split);
    m->stat_enc_plan[0] = plan.per_cu; m->stat_enc_plan[1] = plan.form == PersistEncPlan::NONE ? 0 : plan.grid;
    return plan;
}

template <class Args>
static void fill_persist_enc_args(const casv_model* m, bool packed, float* const* lout, Args& pa) {
    const int W = m->W, D = m->D;
    auto layer = [&](const LstmW& l, int Kt) {
        return packed ? PersistLayer{l.pw.as<float>(), l.pbias.as<float>(), Kt} : PersistLayer{l.wt.as<float>(), l.bias.as<float>(), Kt};
    };
    pa.B = m->B; pa.T = m->T; pa.D = D; pa.W = W;
    pa.l1[0] = layer(m->enc_fw, 2 * W); pa.l1[1] = layer(m->enc_bw, 2 * W);
    for (int n = 2; n <= D; ++n) { pa.ln[n - 2] = layer(m->enc[n], m->enc[n].kin + W); pa.Hn[n - 2] = lout[n]; }
    pa.x0 = m->x0.as<float>(); pa.H1 = m->H1.as<float>(); pa.cfin = m->cfin.as<float>();
    pa.counters = m->p_enc_counters.as<unsigned>();
}

static int launch_persist_enc(casv_model* m, const PersistEncPlan& plan, float* const* lout) {
    std::lock_guard<std::mutex> lock(g_persist_mutex);
    const int T = m->T, W = m->W, D = m->D;
    const size_t BT = (size_t)m->B * T;
    const bool split = plan.form == PersistEncPlan::SPLIT;
    if (int rc = m->p_enc_counters.ensure(plan.counter_bytes)) return rc;
    HIPCHK(hipMemsetAsync(m->p_enc_counters.p, 0, plan.counter_bytes, m->stream));
    PersistEncArgs pc{}; PersistSplitEncArgs ps{};
    if (split) { fill_persist_enc_args(m, false, lout, ps); ps.inject = m->persist_fault_split ? 1 : 0; }
    else { fill_persist_enc_args(m, true, lout, pc); pc.lda = persist_enc_lda(PersistEncShape{D, W, false, false}); }
#ifdef CASV_PERSIST_PROF
    static DevBuf& eprof = *new DevBuf();       // (leaked on purpose: a static DevBuf would free into a runtime that may be gone at exit)
    if (!split) {
        if (int rc = eprof.ensure(32 * 8)) return rc;
        HIPCHK(hipMemsetAsync(eprof.p, 0, 32 * 8, m->stream));
        pc.prof = eprof.as<unsigned long long>();
    }
#endif
    hipEvent_t pev{};
    m->prof_begin(PC_PERSIST, 2.0 * BT * 4.0 * W * (2.0 * 2 * W + (D >= 2 ? 3.0 * W : 0.0) + (D >= 3 ? (D - 2) * 2.0 * W : 0.0)), 0.0, pev);
    persist_order_before(m->device, m->stream);
    if (split ? launch_persist_split_encode(ps, plan.grid, m->stream) : launch_persist_encode(pc, plan.grid, m->stream))
        return fail(CASV_ERR_ARG, "%s", split ? "persistent split encoder: no launch form for this shape" : "persistent encoder: rows do not fit the LDS");
    persist_order_after(m->device, m->stream);
    m->prof_end(PC_PERSIST, pev);
    HIPCHK(hipGetLastError());
#ifdef CASV_PERSIST_PROF
    if (!split) {
        unsigned long long h[32];
        HIPCHK(hipMemcpy(h, eprof.p, sizeof h, hipMemcpyDeviceToHost));
        fprintf(stderr, "persist enc prof (workgroup 0) us/step: phase A wait %.2f stage %.2f kloop %.2f cell %.2f publish %.2f | phase B %.2f %.2f %.2f %.2f %.2f | totals A %.1f us, B %.1f us\n",
                h[0] * 0.01 / T, h[1] * 0.01 / T, h[2] * 0.01 / T, h[3] * 0.01 / T, h[4] * 0.01 / T,
                h[8] * 0.01 / T, h[9] * 0.01 / T, h[10] * 0.01 / T, h[11] * 0.01 / T, h[12] * 0.01 / T, h[16] * 0.01, h[17] * 0.01);
    }
#endif
    return 0;
}

// ---- the per-step forms ----
// One direction of a bidirectional layer at step t (layer 1; with deep_bidirectional_encoder every layer n): inputs x [B][T][kin],
// outputs into its half of H [B][T][2W], cell state of the backward direction in cfin slot n - 1 (the forward one's in a scratch slot)
static GemmArgs bidir_job(const casv_model* m, const LstmW& w, int n, int dir, int t, const float* x, int kin, float* H) {
    const int B = m->B, T = m->T, W = m->W, D = m->D;
    GemmArgs g{};
    const int mul = dir == 0 ? 1 : -1;
    const int addx = dir == 0 ? 0 : T - 1, addh = dir == 0 ? -1 : T;
    g.nseg = 2;
    g.a[0] = mkseg(x, T * kin, kin, 0, nullptr, kin, mul, addx);
    g.a[1] = mkseg(H + dir * W, T * 2 * W, W, kin, nullptr, 2 * W, mul, addh, 1);
    g.Bt = w.wt.as<float>(); g.bias = w.bias.as<float>();
    g.M = B; g.N = 4 * W; g.Ktot = kin + W;
    g.out = mkslot(H + dir * W, T * 2 * W, 2 * W, mul, addx);
    float* cb = m->cfin.as<float>() + (size_t)(dir == 0 ? D : n - 1) * B * W;
    g.c_in = mkseg(cb, W, W, 0, nullptr, 0, 0, 0, 1);
    g.c_out = mkslot(cb, W);
    g.step_imm = t; g.step_ptr = nullptr;
    return g;
}
// Cell t of the unidirectional layer n >= 2: input lout[n - 1], output lout[n], cell state in cfin slot n - 1
static GemmArgs layer_job(const casv_model* m, float* const* lout, int n, int t) {
    const int B = m->B, T = m->T, W = m->W;
    GemmArgs g{};
    const int win = n == 2 ? 2 * W : W;
    g.nseg = 2;
    g.a[0] = mkseg(lout[n - 1], T * win, win, 0, nullptr, win, 1, 0);
    g.a[1] = mkseg(lout[n], T * W, W, win, nullptr, W, 1, -1, 1);
    g.Bt = m->enc[n].wt.as<float>(); g.bias = m->enc[n].bias.as<float>();
    g.M = B; g.N = 4 * W; g.Ktot = win + W;
    g.out = mkslot(lout[n], T * W, W, 1, 0);
    float* cb = m->cfin.as<float>() + (size_t)(n - 1) * B * W;
    g.c_in = mkseg(cb, W, W, 0, nullptr, 0, 0, 0, 1);
    g.c_out = mkslot(cb, W);
    g.step_imm = t;
    return g;
}
// final h of a layer, [B][W] from the layer's output sequence at one position (`src`: row 0 there, `ld` floats per line), into hfin slot n - 1
static bool final_h(const casv_model* m, SmallOps& ops, const float* src, long long ld, int n) {
    return ops.rows(src, ld, m->hfin.as<float>() + (size_t)(n - 1) * m->B * m->W, m->W, m->B, m->W, 1);
}
static int too_many_ops() { return fail(CASV_ERR_STATE, "too many set-up operations for one launch"); }

// Layer 1 on plain text from a per-character table (option "encoder_table").  Every x_t row of such an input is one row of E
// (embed_sparse with one alternative of weight 1) or zeros, so its part of the cell's contraction is one of V + 1 rows -- computed
// B x T times per direction otherwise.  The table holds those rows as the ACCUMULATORS the split GEMM leaves behind the x columns (its
// raw plain output); a cell's job takes its row as GemmArgs.acc_in and contracts the h columns only: the same instruction sequence
// per element as the undivided [x | h] job, the same bits (x comes first in K, its width is whole K tiles, and the 128x128 and
// 256x256 split tiles contract an element alike).
// The table of the committed weights: built on first use by the split GEMM itself, on the handle's stream (never under a
// recording: the encoder pass is not part of the step graph), dropped by casv_commit_weights.
static int ensure_enc_table(casv_model* m) {
    if (m->enc_tab_ready) return 0;
    const int W = m->W, V = m->V;
    const size_t rows = (size_t)V + 1;
    for (int dir = 0; dir < 2; ++dir) if (int rc = m->enc_tab[dir].ensure(rows * 4 * W * 4)) return rc;
    if (int rc = m->enc_tab_x.ensure(rows * W * 4)) return rc;
    if (int rc = m->enc_tab_idx.ensure(rows * 2 * 4)) return rc;
    int* idx = m->enc_tab_idx.as<int>(); float* val = reinterpret_cast<float*>(idx + rows);
    launch_table_input(idx, val, V, m->stream);
    launch_embed_sparse(m->E.as<float>(), idx, val, m->enc_tab_x.as<float>(), (int)rows, 1, V, W, m->stream);      // (the rows a line's x0 holds; row V: zeros)
    GemmBatch b{};
    for (int dir = 0; dir < 2; ++dir) {
        GemmArgs& g = b.g[dir];
        g.nseg = 1; g.a[0] = mkseg(m->enc_tab_x.as<float>(), W, W, 0);
        g.Bt = (dir == 0 ? m->enc_fw : m->enc_bw).wt.as<float>(); g.bias = nullptr;         // (no bias: the raw accumulators)
        g.M = (int)rows; g.N = 4 * W; g.Ktot = 2 * W;
        g.out = mkslot(m->enc_tab[dir].as<float>(), 4 * W);
    }
    b.count = 2;
    run_gemm_batch(m, EPI_PLAIN, b);
    HIPCHK(hipGetLastError());
    m->enc_tab_ready = true;
    ++m->stat_enc_table_builds;
    return 0;
}
// a layer-1 job on the table: the h columns alone, on top of the row of the position's character (chars: [T][B], V = none)
static GemmArgs table_job(const casv_model* m, int dir, int t, const int* chars) {
    GemmArgs g = bidir_job(m, dir == 0 ? m->enc_fw : m->enc_bw, 1, dir, t, m->x0.as<float>(), m->W, m->H1.as<float>());
    const int pos = dir == 0 ? t : m->T - 1 - t;
    g.a[0] = g.a[1]; g.a[1] = Seg{}; g.nseg = 1;            // (koff of the h columns and the weights' row stride Ktot stay)
    g.acc_in = mkseg(m->enc_tab[dir].as<float>(), 4 * m->W, 0, 0, chars + (size_t)pos * m->B);
    return g;
}
// Whether this pass takes the table: the option, the split arithmetic, plain-text input, no bridge -- and every launch of a step in
// the one form that honours acc_in (gemm_plan.h)
static bool layer1_takes_table(casv_model* m) {
    if (m->enc_table_opt < 1 || m->gemm.arithmetic < 1 || !m->enc_onehot || m->A != 1 || m->cfg.bridge_dense) return false;
    GemmBatch b{};
    const int* any = reinterpret_cast<const int*>(m->d_idx.p);
    for (int dir = 0; dir < 2; ++dir) b.g[dir] = table_job(m, dir, 0, any);
    b.count = 2;
    return gemm_plan_takes_acc_in(plan_gemm_launches(m->gemm, gemm_switches(), EPI_LSTM, b));
}

// layer 1 (seq2seq.py:272-281): the forward step at time t and the backward step at time T-1-t are independent -> one launch of two jobs
static int run_layer1_steps(casv_model* m, bool table = false) {
    const int* chars = nullptr;
    if (table) {
        if (int rc = ensure_enc_table(m)) return rc;
        if (int rc = m->enc_cidx.ensure((size_t)m->B * m->T * 4)) return rc;
        launch_char_rows(m->d_idx.as<int>(), m->enc_cidx.as<int>(), m->B, m->T, m->V, m->stream);
        chars = m->enc_cidx.as<int>();
    }
    m->stat_enc_table = table ? 1 : 0;
    for (int t = 0; t < m->T; ++t) {
        GemmBatch b{};
        for (int dir = 0; dir < 2; ++dir)
            b.g[dir] = table ? table_job(m, dir, t, chars)
                             : bidir_job(m, dir == 0 ? m->enc_fw : m->enc_bw, 1, dir, t, m->x0.as<float>(), m->W, m->H1.as<float>());
        b.count = 2;
        run_gemm_batch(m, EPI_LSTM, b);
    }
    return 0;
}
// layers 2..D (seq2seq.py:283): cell (n, t) needs (n-1, t) and (n, t-1); the cells of one anti-diagonal k = t + (n-2) are
// independent -> one launch per diagonal (<= GEMM_MAX_JOBS cells, deeper stacks are cut into groups of GEMM_MAX_JOBS layers)
static void run_wavefront(casv_model* m, float* const* lout) {
    const int T = m->T, D = m->D;
    for (int n0 = 2; n0 <= D; n0 += GEMM_MAX_JOBS) {
        const int n1 = std::min(D, n0 + GEMM_MAX_JOBS - 1);
        for (int k = 0; k < T + (n1 - n0); ++k) {
            GemmBatch b{};
            for (int n = n0; n <= n1; ++n) {
                const int t = k - (n - n0);
                if (t >= 0 && t < T) b.g[b.count++] = layer_job(m, lout, n, t);
            }
            run_gemm_batch(m, EPI_LSTM, b);
        }
    }
}
// Option "encoder_table" = 2: the input terms of layers 2..D ahead of their recurrence.  The x part of all T cells of layer n is known
// once layer n - 1 has finished: ONE plain contraction of M = B * T rows (no bias: the raw accumulators, on whatever split tiles fill
// the chip) into enc_zx [B][T][4W]; cell t then takes its rows as acc_in and contracts h alone -- the same bits, as for layer 1's table.
// This gives up the anti-diagonal: the layers run one after the other, each as T launches of ONE job of K = W.
static GemmArgs ahead_job(const casv_model* m, float* const* lout, int n, int t) {
    GemmArgs g = layer_job(m, lout, n, t);
    g.a[0] = g.a[1]; g.a[1] = Seg{}; g.nseg = 1;            // (koff of the h columns and the weights' row stride Ktot stay)
    g.acc_in = mkseg(m->enc_zx.as<float>(), m->T * 4 * m->W, 0, 0, nullptr, 4 * m->W, 1, 0);
    return g;
}
static bool upper_layers_take_ahead(casv_model* m, float* const* lout) {
    if (m->enc_table_opt < 2 || m->gemm.arithmetic < 1 || m->cfg.bridge_dense || m->D < 2) return false;
    GemmBatch b{};
    b.g[0] = ahead_job(m, lout, 2, 0); b.count = 1;
    if (!b.g[0].acc_in.base) b.g[0].acc_in.base = m->H1.as<float>();        // (planned before the buffer exists: any non-null address)
    return gemm_plan_takes_acc_in(plan_gemm_launches(m->gemm, gemm_switches(), EPI_LSTM, b));
}
static int run_layers_ahead(casv_model* m, float* const* lout) {
    const int B = m->B, T = m->T, W = m->W;
    if (int rc = m->enc_zx.ensure((size_t)B * T * 4 * W * 4)) return rc;
    for (int n = 2; n <= m->D; ++n) {
        const int win = n == 2 ? 2 * W : W;
        GemmArgs x{};
        x.nseg = 1; x.a[0] = mkseg(lout[n - 1], win, win, 0);
        x.Bt = m->enc[n].wt.as<float>(); x.bias = nullptr;
        x.M = B * T; x.N = 4 * W; x.Ktot = win + W;
        x.out = mkslot(m->enc_zx.as<float>(), 4 * W);
        run_gemm(m, EPI_PLAIN, x);
        for (int t = 0; t < T; ++t) { GemmArgs g = ahead_job(m, lout, n, t); run_gemm(m, EPI_LSTM, g); }
    }
    m->stat_enc_ahead = 1;
    return 0;
}
// residual_connections (seq2seq.py:284-291): from layer 3 on a layer's output sequence is its LSTM output plus its input sequence
// -- no wavefront across such layers: they run one after the other, the sum is taken in place over the whole sequence once a
// layer has finished (its final h -- the LSTM's own -- set aside first)
static int run_residual_layers(casv_model* m, float* const* lout) {
    const int T = m->T, W = m->W;
    for (int n = 2; n <= m->D; ++n) {
        for (int t = 0; t < T; ++t) { GemmArgs g = layer_job(m, lout, n, t); run_gemm(m, EPI_LSTM, g); }
        SmallOps ops{};
        final_h(m, ops, lout[n] + (size_t)(T - 1) * W, (long long)T * W, n);
        if (!launch_small_ops(ops, m->stream)) return too_many_ops();
        if (n >= 3) launch_add_inplace(lout[n], lout[n - 1], (long long)m->B * T * W, m->stream);
    }
    return 0;
}
// deep_bidirectional_encoder (seq2seq.py:246-281): every layer n >= 2 is bidirectional too, reads the "cross sum" of the layer below
// (each pair of neighbouring features of [fw | bw] replaced by its sum) and hands on its BACKWARD final state -- layer after
// layer (a backward direction ends where the next layer starts), two jobs per launch; the outputs alternate between H1 and a
// buffer of their own.  *out: the last layer's.
static int run_deep_layers(casv_model* m, float** out) {
    const int T = m->T, W = m->W;
    const size_t BT = (size_t)m->B * T;
    if (int rc = m->Hc.ensure((size_t)2 * BT * 2 * W * 4)) return rc;
    float* H1 = m->H1.as<float>(); float* bufA = m->Hc.as<float>(); float* xs = bufA + (size_t)BT * 2 * W;
    float* prev = H1;
    for (int n = 1; n <= m->D; ++n) {
        float* H = prev;
        if (n >= 2) {
            H = prev == H1 ? bufA : H1;
            launch_cross_sum(prev, xs, (long long)BT * 2 * W, m->stream);
            for (int t = 0; t < T; ++t) {
                GemmBatch b{};
                b.g[0] = bidir_job(m, m->enc_dfw[n], n, 0, t, xs, 2 * W, H); b.g[1] = bidir_job(m, m->enc_dbw[n], n, 1, t, xs, 2 * W, H); b.count = 2;
                run_gemm_batch(m, EPI_LSTM, b);
            }
        }
        SmallOps ops{};         // backward final h of layer n = its output at time 0 (layer 1's now: its buffer takes layer 3's outputs)
        final_h(m, ops, H + W, (long long)T * 2 * W, n);
        if (!launch_small_ops(ops, m->stream)) return too_many_ops();
        prev = H;
    }
    *out = prev;
    return 0;
}

// bridge_dense (seq2seq.py:299-301): the final states through Dense(width, tanh) on their way to the decoder
static int run_bridges(casv_model* m) {
    const int W = m->W;
    const size_t BW = (size_t)m->B * W;
    if (int rc = m->br_tmp.ensure(BW * 4)) return rc;
    for (int n = 1; n <= m->D; ++n)
        for (int s = 0; s < 2; ++s) {
            float* st = (s ? m->cfin.as<float>() : m->hfin.as<float>()) + (size_t)(n - 1) * BW;
            GemmArgs g{};
            g.nseg = 1; g.a[0] = mkseg(st, W, W, 0);
            g.Bt = (s ? m->br_cT[n] : m->br_hT[n]).as<float>(); g.bias = (s ? m->br_cb[n] : m->br_hb[n]).as<float>();
            g.M = m->B; g.N = W; g.Ktot = W;
            g.out = mkslot(m->br_tmp.as<float>(), W);
            run_gemm(m, EPI_PLAIN, g);
            launch_tanh(m->br_tmp.as<float>(), st, (long long)BW, m->stream);
        }
    return 0;
}

// u = attention_dense(enc_out) once per line (seq2seq.py:313,459-460; the reference redoes it every step)
static void attention_dense(casv_model* m) {
    GemmArgs g{};
    g.nseg = 1; g.a[0] = mkseg(m->enc_out, m->C, m->C, 0);
    g.Bt = m->UT.as<float>(); g.bias = nullptr; g.M = m->B * m->T; g.N = m->W; g.Ktot = m->C;
    g.out = mkslot(m->u.as<float>(), m->W);
    run_gemm(m, EPI_PLAIN, g);
}

// The encoder (seq2seq.py:237-314) on the inputs that lie in d_idx / d_val: embedding, BiLSTM layer, stacked layers, final states,
// u = attention_dense(enc_out).  Small batches: the whole recurrence as ONE persistent launch -- whose give-up word is NOT waited
// for here: it is copied aside (d_flags[0]) and looked at where the host waits for the device anyway (settle_encoder: the end of
// the greedy decode, or the first other consumer of the outputs); a launch that gave up is redone with the per-step kernels then.
// (Waiting here cost every batch of configs[1] a host round trip with the GPU idle between its encoder and its decoder's set-up.)
static int run_encoder(casv_model* m, bool try_persistent) {
    SplitScope arithmetic(m, m->enc_arith < 0 ? 0 : m->enc_arith);   // (set by ensure_encoded; its own scope: settle_encoder redoes an encoder from inside any entry point)
    const int B = m->B, T = m->T, A = m->A, W = m->W, D = m->D;
    const size_t BT = (size_t)B * T;
    if (int rc = m->d_flags.ensure(64)) return rc;
    enum { PERSISTENT, WAVEFRONT, RESIDUAL, DEEP } form = WAVEFRONT;
    PersistEncPlan plan{};
    if (try_persistent) plan = plan_persist_enc(m, B);
    if (plan.form != PersistEncPlan::NONE && !persist_backed_off(m->persist_backoff)) form = PERSISTENT;
    else if (m->cfg.deep_bidirectional_encoder && D >= 2) form = DEEP;
    else if (m->cfg.residual_connections && D >= 3) form = RESIDUAL;       // (the sums live in the unidirectional branch, seq2seq.py:282-291)

    m->stat_enc_table = 0; m->stat_enc_ahead = 0;
    // (layer 1 from the per-character table reads the characters, not x0: no embedding launch then)
    const bool table = form == WAVEFRONT && layer1_takes_table(m);
    if (!table) {
        hipEvent_t ev{};
        m->prof_begin(PC_EMBED, 2.0 * BT * A * W, 4.0 * BT * W * (A + 1), ev);
        launch_embed_sparse(m->E.as<float>(), m->d_idx.as<int>(), m->d_val.as<float>(), m->x0.as<float>(), (int)BT, A, m->V, W, m->stream);
        m->prof_end(PC_EMBED, ev);
    }

    // outputs of layer n: layers that run strictly one after another alternate between two buffers (depth <= 3), deeper stacks
    // have a slice each of one buffer; the deep form plans its own
    float* H1 = m->H1.as<float>();
    float* lout[9] = {nullptr, H1};
    if (form != DEEP) {
        if (D >= 4) { if (int rc = m->Hc.ensure((size_t)(D - 1) * BT * W * 4)) return rc; }
        for (int n = 2; n <= D; ++n)
            lout[n] = D >= 4 ? m->Hc.as<float>() + (size_t)(n - 2) * BT * W : (n % 2 == 0) ? m->Ha.as<float>() : m->Hb.as<float>();
    }
    float* out = lout[D];
    unsigned* give_up = nullptr;
    switch (form) {
        case PERSISTENT:
            if (int rc = launch_persist_enc(m, plan, lout)) return rc;
            give_up = persist_give_up_word(m->p_enc_counters.as<unsigned>(), plan.counter_bytes);
            break;
        case WAVEFRONT:
            if (int rc = run_layer1_steps(m, table)) return rc;
            if (upper_layers_take_ahead(m, lout)) { if (int rc = run_layers_ahead(m, lout)) return rc; }
            else run_wavefront(m, lout);
            break;
        case RESIDUAL: (void)run_layer1_steps(m); if (int rc = run_residual_layers(m, lout)) return rc; break;
        case DEEP: (void)run_layer1_steps(m); if (int rc = run_deep_layers(m, &out)) return rc; break;
    }
    {   // final hidden states that no form above has set aside, and the persistent launch's give-up word, in one launch:
        // backward final h of layer 1 = its output at time 0 (seq2seq.py:280); layers n >= 2: the output at the last position
        SmallOps ops{};
        if (form != DEEP) final_h(m, ops, H1 + W, (long long)T * 2 * W, 1);
        for (int n = 2; n <= D && (form == PERSISTENT || form == WAVEFRONT); ++n) final_h(m, ops, lout[n] + (size_t)(T - 1) * W, (long long)T * W, n);
        if (give_up) ops.rows(reinterpret_cast<const float*>(give_up), 1, m->d_flags.as<float>(), 1, 1, 1, 1);
        if (!launch_small_ops(ops, m->stream)) return too_many_ops();
    }
    m->enc_check_pending = form == PERSISTENT;
    m->stat_enc_persistent = form == PERSISTENT ? 1 : 0;
    if (m->cfg.bridge_dense) if (int rc = run_bridges(m)) return rc;
    m->enc_out = out;
    attention_dense(m);
    HIPCHK(hipGetLastError());
    return CASV_OK;
}

// The persistent encoder's give-up word, where the host has to wait for the device anyway.  `have_flag`: the caller has already
// brought d_flags[0] to the host (value in *flag) behind a synchronisation of its own; otherwise this function does both.
// A launch that gave up (its workgroups were not all resident: another process's persistent kernel on this GPU) is redone with the
// per-step kernels -- same values.  Returns 1 if the encoder was redone (whatever was decoded from its outputs must be redone too).
int settle_encoder(casv_model* m, const unsigned* flag) {
    if (!m->enc_check_pending) return 0;
    unsigned aborted = 0;
    if (flag) aborted = *flag;
    else {
        HIPCHK(hipMemcpyAsync(&aborted, m->d_flags.p, 4, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    m->enc_check_pending = false;
    if (!aborted) { if (!flag) m->persist_backoff.penalty = 0; return 0; }      // (with `flag` the caller has a second launch to account for before the back-off is reset)
    persist_note_abort(m->persist_backoff, "encoder");
    ++m->stat_decode_give_ups;          // (statistic "decode_give_ups")
    if (int rc = run_encoder(m, false)) return rc;      // (also takes the statistic "encoder_persistent" back)
    return 1;
}

// The encoder outputs in the arithmetic of the entry point that is about to consume them (engine.h, arithmetic_of): computed at the
// first such call after casv_encode / casv_set_encoder_outputs, kept for further calls of the same arithmetic, redone for the other.
int ensure_encoded(casv_model* m, int want) {
    if (m->enc_arith == want) { m->stat_enc_persistent = 0; return 0; }     // (an encoding that is reused)
    m->enc_check_pending = false;
    m->stat_enc_persistent = 0;
    m->enc_arith = want;                // (run_encoder reads it; taken back on every failure: the outputs on the device are then nobody's)
    if (!m->enc_explicit) {
        if (int rc = run_encoder(m, true)) { m->enc_arith = -1; return rc; }
        return 0;
    }
    SplitScope arithmetic(m, want);        // (on outputs that were handed in)
    attention_dense(m);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) { m->enc_arith = -1; return fail(CASV_ERR_HIP, "attention_dense launch failed: %s", hipGetErrorString(e)); }
    return 0;
}

extern "C" int casv_encode(casv_model* m, int32_t B, int32_t T, int32_t A, const int32_t* idx, const float* val,
                           const int32_t* src_rej) {
    if (!m || !idx || !val) return fail(CASV_ERR_ARG, "null argument");
    if (!m->committed) return fail(CASV_ERR_STATE, "weights not committed");
    if (B < 1 || T < 1 || A < 1) return fail(CASV_ERR_ARG, "bad shape B=%d T=%d A=%d", B, T, A);
    if (T > CASV_MAX_T) return fail(CASV_ERR_ARG, "line length %d exceeds the supported maximum of %d", T, CASV_MAX_T);
    HIPCHK(hipSetDevice(m->device));
    const int W = m->W, D = m->D;
    const size_t BT = (size_t)B * T;
    if (int rc = m->d_idx.ensure(BT * A * 4)) return rc;
    if (int rc = m->d_val.ensure(BT * A * 4)) return rc;
    if (int rc = m->d_srcrej.ensure(BT * 4)) return rc;
    if (int rc = m->x0.ensure(BT * W * 4)) return rc;
    if (int rc = m->H1.ensure(BT * 2 * W * 4)) return rc;
    if (D == 2 || D == 3) { if (int rc = m->Ha.ensure(BT * W * 4)) return rc; }
    if (D == 3) { if (int rc = m->Hb.ensure(BT * W * 4)) return rc; }
    if (int rc = m->cfin.ensure((size_t)(D + 1) * B * W * 4)) return rc;     // slot D: forward c of layer 1 (unused later)
    if (int rc = m->hfin.ensure((size_t)D * B * W * 4)) return rc;
    if (int rc = m->u.ensure(BT * W * 4)) return rc;
    // The caller owns idx / val / src_rej and may release them as soon as this function returns (the encoder itself runs
    // asynchronously).  They are copied into a pinned staging buffer of the handle first: the device copies then need no wait --
    // the function returns while they are still queued (waiting for pageable copies cost every batch of configs[1] ~40 us of idle
    // GPU) -- and the staging buffer is reused only once its previous copies have gone (ev_inputs).
    const size_t nin = BT * A * 4, nrej = BT * 4, need = 2 * nin + nrej;
    if (need > m->pin_limit) {
        // (very large inputs: no pinned copy of that size -- straight from the caller's buffers, and wait until they have been read)
        HIPCHK(hipMemcpyAsync(m->d_idx.p, idx, nin, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->d_val.p, val, nin, hipMemcpyHostToDevice, m->stream));
        if (src_rej) HIPCHK(hipMemcpyAsync(m->d_srcrej.p, src_rej, nrej, hipMemcpyHostToDevice, m->stream));
        else HIPCHK(hipMemsetAsync(m->d_srcrej.p, 0xff, nrej, m->stream));
        HIPCHK(hipEventRecord(m->ev_inputs, m->stream));
        HIPCHK(hipEventSynchronize(m->ev_inputs));
    } else {
    if (m->pin_in_cap < need) {
        if (m->pin_in) { HIPCHK(hipStreamSynchronize(m->stream)); (void)hipHostFree(m->pin_in); m->pin_in = nullptr; m->pin_in_cap = 0; }
        HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&m->pin_in), need, hipHostMallocDefault));
        m->pin_in_cap = need;
    } else HIPCHK(hipEventSynchronize(m->ev_inputs));
    memcpy(m->pin_in, idx, nin); memcpy(m->pin_in + nin, val, nin);
    if (src_rej) memcpy(m->pin_in + 2 * nin, src_rej, nrej);
    HIPCHK(hipMemcpyAsync(m->d_idx.p, m->pin_in, nin, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->d_val.p, m->pin_in + nin, nin, hipMemcpyHostToDevice, m->stream));
    if (src_rej) HIPCHK(hipMemcpyAsync(m->d_srcrej.p, m->pin_in + 2 * nin, nrej, hipMemcpyHostToDevice, m->stream));
    else HIPCHK(hipMemsetAsync(m->d_srcrej.p, 0xff, nrej, m->stream));
    HIPCHK(hipEventRecord(m->ev_inputs, m->stream));
    }
    m->B = B; m->T = T; m->A = A;
    // plain text: one alternative per position, of weight exactly 1 where there is a character (layer 1 may then come from the
    // per-character table, run_layer1_steps)
    m->enc_onehot = A == 1 && m->enc_table_opt >= 1;        // (looked at only where the table can be taken at all)
    for (size_t i = 0; i < BT && m->enc_onehot; ++i) if (idx[i] >= 0 && idx[i] < m->V && val[i] != 1.0f) m->enc_onehot = false;
    m->last_decode = 0; m->has_a0 = false;
    m->enc_check_pending = false;
    // The encoder itself runs for the first entry point that needs its outputs, in that entry point's arithmetic (ensure_encoded):
    // what a search returns for a line must not depend on whether somebody looked at the encoder outputs or decoded greedily before.
    m->enc_arith = -1; m->enc_explicit = false;
    m->encoded = true;
    return CASV_OK;
}

extern "C" int casv_set_encoder_outputs(casv_model* m, int32_t B, int32_t T, const float* enc_out, const float* states,
                                        const float* a0, const int32_t* src_rej) {
    if (!m || !enc_out || !states) return fail(CASV_ERR_ARG, "null argument");
    if (!m->committed) return fail(CASV_ERR_STATE, "weights not committed");
    if (B < 1 || T < 1) return fail(CASV_ERR_ARG, "bad shape B=%d T=%d", B, T);
    if (T > CASV_MAX_T) return fail(CASV_ERR_ARG, "line length %d exceeds the supported maximum of %d", T, CASV_MAX_T);
    HIPCHK(hipSetDevice(m->device));
    const int W = m->W, C = m->C, D = m->D;
    const size_t BT = (size_t)B * T, BW = (size_t)B * W;
    if (int rc = m->Hc.ensure(std::max((size_t)(D - 1), (size_t)1) * BT * std::max(W, C) * 4)) return rc;
    if (int rc = m->d_srcrej.ensure(BT * 4)) return rc;
    if (int rc = m->cfin.ensure((size_t)(D + 1) * BW * 4)) return rc;
    if (int rc = m->hfin.ensure((size_t)D * BW * 4)) return rc;
    if (int rc = m->u.ensure(BT * W * 4)) return rc;
    m->enc_out = m->Hc.as<float>();
    HIPCHK(hipMemcpyAsync(m->enc_out, enc_out, BT * C * 4, hipMemcpyHostToDevice, m->stream));
    for (int n = 0; n < D; ++n) {
        HIPCHK(hipMemcpyAsync(m->hfin.as<float>() + n * BW, states + (size_t)(2 * n) * BW, BW * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipMemcpyAsync(m->cfin.as<float>() + n * BW, states + (size_t)(2 * n + 1) * BW, BW * 4, hipMemcpyHostToDevice, m->stream));
    }
    if (src_rej) HIPCHK(hipMemcpyAsync(m->d_srcrej.p, src_rej, BT * 4, hipMemcpyHostToDevice, m->stream));
    else HIPCHK(hipMemsetAsync(m->d_srcrej.p, 0xff, BT * 4, m->stream));
    m->has_a0 = a0 != nullptr;
    if (a0) {
        if (int rc = m->a0.ensure(BT * 4)) return rc;
        HIPCHK(hipMemcpyAsync(m->a0.p, a0, BT * 4, hipMemcpyHostToDevice, m->stream));
    }
    HIPCHK(hipEventRecord(m->ev_inputs, m->stream));
    HIPCHK(hipEventSynchronize(m->ev_inputs));
    m->B = B; m->T = T; m->A = 1;
    m->last_decode = 0; m->enc_check_pending = false;
    m->enc_arith = -1; m->enc_explicit = true;         // u = attention_dense(enc_out) follows in the consumer's arithmetic (ensure_encoded)
    m->encoded = true;
    return CASV_OK;
}

extern "C" int casv_get_encoder_outputs(casv_model* m, float* enc_out, float* states) {
    if (!m) return fail(CASV_ERR_ARG, "null argument");
    if (!m->encoded) return fail(CASV_ERR_STATE, "nothing encoded");
    HIPCHK(hipSetDevice(m->device));
    if (int rc = ensure_encoded(m, arithmetic_of(m, ENTRY_CHAIN))) return rc;
    if (int rc = settle_encoder(m); rc < 0) return rc;
    HIPCHK(hipStreamSynchronize(m->stream));
    const size_t BW = (size_t)m->B * m->W;
    if (enc_out) HIPCHK(hipMemcpy(enc_out, m->enc_out, (size_t)m->B * m->T * m->C * 4, hipMemcpyDeviceToHost));
    if (states)
        for (int n = 0; n < m->D; ++n) {
            HIPCHK(hipMemcpy(states + (2 * n) * BW, m->hfin.as<float>() + n * BW, BW * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(states + (2 * n + 1) * BW, m->cfin.as<float>() + n * BW, BW * 4, hipMemcpyDeviceToHost));
        }
    return CASV_OK;
}

// Test support: u = attention_dense(enc_out) [B][T][W] as the last encoder pass left it on the device (CASV_ERR_STATE before one has run)
extern "C" int casv_debug_get_u(casv_model* m, float* u) {
    if (!m || !u) return fail(CASV_ERR_ARG, "null argument");
    if (!m->encoded || m->enc_arith < 0) return fail(CASV_ERR_STATE, "no encoder pass has run on this input");
    HIPCHK(hipSetDevice(m->device));
    if (int rc = settle_encoder(m); rc < 0) return rc;
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipMemcpy(u, m->u.p, (size_t)m->B * m->T * m->W * 4, hipMemcpyDeviceToHost));
    return CASV_OK;
}
