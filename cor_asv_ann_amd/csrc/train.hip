// Teacher-forced train step on the device: kt:195 `model.train_on_batch` / kt:407 `test_on_batch` of the
// graph `encoder_decoder_model` (seq2seq.py:237-390) compiled with weighted categorical cross-entropy and
// Adam(clipnorm=5) (seq2seq.py:494-497), plus the embedding regulariser (seq2seq.py:530-553).
//
// Layout: every sequence tensor is time-major [t][b][f].  Per LSTM layer the parameters are split into
//   Wx [4W][kx]  input part   -> ONE GEMM over all time steps gives the input pre-activations (+ bias)
//   Wr [4W][kr]  recurrent part (attention cell: [context | h]) -> one fused LSTM-cell GEMM per step
// rows in the gate-interleaved order of gemm.hip.  Backward per step = pointwise cell backward + one
// data GEMM through the recurrent part; input gradients and all weight gradients are big GEMMs over
// the whole sequence (operands transposed by a bandwidth-bound kernel).  Adam and the global-norm clip
// run on these packed tensors; Keras layouts exist only at set/get time.
//
// casv_train_step fills the step's view (Step) and makes at most two attempts (train_attempt); an attempt is these phases, in order:
//   1 plan_buffers     every buffer large enough for the step's shapes, the layers' output places
//   2 stage_inputs     batch, masks, segments on the device; sums, counters, gradients cleared; the per-step state reset
//   3 forward_layers   encoder stack beside the decoder layers below the cell; final states, bridges, u
//   4 forward_cell     attention cell
//   5 loss_head        projection, softmax cross-entropy (training: dL/dlogits)        -- give-up check; mode 0 ends here
//   6 backward_cell    tied projection, attention cell, the cell's and the attention's parameters
//   7 backward_layers  decoder / encoder pairs downwards, embedding                    -- give-up check
//   8 update           regulariser, norm, clipped Adam, results
// train_plan.h decides and counts the persistent launches of a step; persist_launch is the one place that asks it and launches.
// casv_train_step_soft is the same step on soft targets: K (index, mass) slots per position (Step::K / soft_idx / soft_q) staged in
// place of the target indices in phase 2, the soft head's launcher in phase 5; every other phase does not know the difference.
// casv_train_step_sampled (train_sched.hip) is the same step with scheduled sampling: sched_passes between phases 4 and 5 (Step::sched),
// which leaves the last pass's tape where phase 4 leaves the teacher-forced one; every later phase does not know the difference.
// The state the step works on is train_state.h / train_state.hip; Step and the phases a scoring call shares are declared in train_step.h.
#include "train_step.h"

namespace casv {

// CASV_ATTN_DEFER and CASV_TOPB_SPLIT, read once, as train_plan.h takes them.
// CASV_ATTN_DEFER: d_enc / du summed behind the cell's backward recurrence instead of by float atomics inside it (attn_bwd.h,
// DEFER; the recurrence has forms 0, 1 and 3 only).  CASV_TOPB_SPLIT: the attention backward of the samples as a launch of its own on
// a second stream, resident beside the big one: it then runs under the h tiles instead of behind them (CASV_TOPB_SPLIT=0: one launch).
// Two launches that hand rows to each other must be resident TOGETHER: where the runtime serialises kernel dispatch
// (rocprofv3 --pmc sets ROCPROF_COUNTERS; AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING) the side launch would never see
// the main one's counters -- one launch there, said once on stderr (profiles taken that way describe that form).
static TrainSwitches read_train_switches() {
    TrainSwitches sw{1, true};
    if (const char* e = getenv("CASV_ATTN_DEFER")) { const int v = atoi(e); sw.defer = v == 3 ? 3 : v == 0 ? 0 : 1; }
    const char* e = getenv("CASV_TOPB_SPLIT");
    if (e && e[0] == '0') { sw.split = false; return sw; }
    auto on = [](const char* name) { const char* v = getenv(name); return v && v[0] && !(v[0] == '0' && !v[1]); };
    const char* why = getenv("ROCPROF_COUNTERS") ? "ROCPROF_COUNTERS (counter collection)" : on("AMD_SERIALIZE_KERNEL") ? "AMD_SERIALIZE_KERNEL" :
                      on("HIP_LAUNCH_BLOCKING") ? "HIP_LAUNCH_BLOCKING" : nullptr;
    if (why && !(e && e[0] == '1')) {       // (CASV_TOPB_SPLIT=1 insists)
        fprintf(stderr, "cor_asv_ann_hip: kernel dispatch is serialised (%s): the attention cell's backward runs as ONE launch "
                        "(the two-launch form needs both resident together)\n", why);
        sw.split = false;
    }
    return sw;
}

// The one place that asks train_plan.h whether a site of the step goes persistent, and launches it if so.  It hands the plan what
// only the device and the environment know -- the residency figure of the kind's kernel, and for the cell's backward the switches
// and whether its two launches fit a CU -- where the step's gate is open at all; `launch(plan, counters)` fills the kernel's
// arguments and issues it (0 or an error) inside the PC_PERSIST bracket; the launch's give-up word is noted for recurrences_gave_up.
// *persistent: the site ran this way -- else the caller takes its per-step form.
static TrainSite persist_site(TrainKind kind, const TrainShape& shape, bool plain = true, int T = 0) {
    return TrainSite{kind, shape, 0, plain, T, TrainSwitches{0, false}, false, false};
}
template <class Launch>
static int persist_launch(casv_model* m, TrainSite site, double flops, bool* persistent, Launch&& launch) {
    TrainState* ts = m->train;
    *persistent = false;
    const TrainGate gate{m->persist_mode, m->deterministic, ts->rec_skip != 0, m->ncu};
    if (train_gate_open(gate) && site.plain) {
        const int W = site.shape.W;
        site.per_cu = site.kind == TRAIN_REC ? train_recurrence_blocks_per_cu(W) : site.kind == TRAIN_REC_BWD ? train_recurrence_bwd_blocks_per_cu(W)
                    : site.kind == TRAIN_CELL ? train_attention_cell_blocks_per_cu(W) : train_attention_cell_bwd_blocks_per_cu(W);
        if (site.kind == TRAIN_CELL_BWD) {
            static const TrainSwitches sw = read_train_switches();
            site.sw = sw; site.split_off = ts->split_off;
            site.rows_fit = train_attention_cell_bwd_rows_fit(W);
        }
    }
    const TrainLaunch plan = ts->plan.next(gate, site);
    if (!plan.persistent) return 0;
    unsigned* counters = reinterpret_cast<unsigned*>(static_cast<char*>(ts->rec_cnt.p) + plan.slot_offset);
    hipEvent_t ev{};
    m->prof_begin(PC_PERSIST, flops, 0.0, ev);
    if (int rc = launch(plan, counters)) return rc;
    m->prof_end(PC_PERSIST, ev);
    ts->rec_abort[plan.slot] = persist_give_up_word(counters, plan.counter_bytes);
    *persistent = true;
    return 0;
}

static GemmArgs plain_gemm(const float* A, long long lda, int M, int K, const float* Bt, int N, const float* bias, float* C_, long long ldc,
                           int accumulate = 0) {
    GemmArgs g{};
    g.nseg = 1; g.a[0] = mkseg(A, (int)lda, K, 0);
    g.Bt = Bt; g.bias = bias; g.M = M; g.N = N; g.Ktot = K;
    g.out = mkslot(C_, (int)ldc); g.accumulate = accumulate; g.ksplit = -1; g.kgroups = 2;
    return g;
}

// A plain contraction over the whole sequence (thousands of rows, nothing fused): through the vendor library when that is switched
// on and has a solution for the shape (vendor_gemm.hip), else gemm.hip.
static void run_plain(casv_model* m, GemmArgs& g) {
#ifdef CASV_GEMM_PROF_PLAIN
    {   // diagnostic build: stamps of every plain whole-sequence contraction, one line per launch (M, N, K)
        (void)hipStreamSynchronize(m->stream);
        casv::gemm_prof_dump();
        fprintf(stderr, "plain gemm M=%d N=%d K=%d accumulate=%d\n", g.M, g.N, g.Ktot, g.accumulate);
    }
#endif
    if (m->vendor_gemm && !m->deterministic && g.nseg == 1 && !g.a[0].rows && !g.step_ptr && g.M >= 4096 && g.a[0].width == g.Ktot && g.a[0].koff == 0) {
        hipEvent_t ev{};
        m->prof_begin(PC_GEMM, 2.0 * g.M * (double)g.N * g.Ktot, 4.0 * ((double)g.M * g.Ktot + (double)g.N * g.Ktot + (double)g.M * g.N), ev);
        const bool done = vendor_gemm_nt(g.a[0].base, g.a[0].ld, g.M, g.Ktot, g.Bt, g.N, g.bias, g.out.base, g.out.ld, g.accumulate, m->stream);
        m->prof_end(PC_GEMM, ev);
        if (done) return;
    }
    run_gemm(m, EPI_PLAIN, g);
}

// C[M][N] += A^T . B for operands as the forward / backward passes left them: A [K][lda], B [K][ldb] (gemm_tn.hip)
static void run_gemm_tn(casv_model* m, const float* A, long long lda, int M, int Mstore, const float* B, long long ldb, int N, long long K,
                        float* C, long long ldc, float* colsum = nullptr) {
    TnArgs g{};
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = M; g.Mstore = Mstore; g.N = N; g.K = (int)K; g.accumulate = 1;
    g.colsum = colsum;
    hipEvent_t ev{};
    m->prof_begin(PC_GEMM, 2.0 * Mstore * (double)N * (double)K, 4.0 * ((double)K * (M + N) + (double)Mstore * N), ev);
    // (the step's arithmetic, engine.h ENTRY_TRAIN: the big weight gradients on bf16x3-split operands where the shape has that form)
    if (m->deterministic) {             // K shares from the shape alone, their partials added in share order (gemm_tn.hip)
        const size_t bytes = gemm_tn_ordered_floats(m->gemm, g) * sizeof(float);
        TrainState* ts = m->train;
        if (bytes > ts->tn_ws.cap) {
            (void)hipStreamSynchronize(m->stream);
            if (int rc = ts->tn_ws.ensure(bytes)) { if (!ts->tn_ws_rc) ts->tn_ws_rc = rc; m->prof_end(PC_GEMM, ev); return; }
        }
        (void)launch_gemm_tn_any(m->gemm, g, ts->tn_ws.as<float>(), m->stream);
    } else (void)launch_gemm_tn_any(m->gemm, g, nullptr, m->stream);
    m->prof_end(PC_GEMM, ev);
}

// One recurrent step of a layer as a GEMM job; k = processing index (time t = k, or len-1-k when reversed).
static GemmArgs layer_step_job(casv_model* m, TLayer& l, int k, const float* h0, const float* c0, const float* rec_in /*top cell*/) {
    TrainState* ts = m->train;
    const int W = m->W, B = l.rows;
    const int mul = l.reverse ? -1 : 1, add_t = l.reverse ? l.len - 1 : 0, add_p = l.reverse ? l.len : -1;
    GemmArgs g{};
    g.nseg = 1;
    if (rec_in) g.a[0] = mkseg(rec_in, l.kr, l.kr, 0, nullptr, (long long)B * l.kr, 1, 0);
    else {
        g.a[0] = mkseg(l.hs, (int)l.hs_ld, W, 0, nullptr, (long long)B * l.hs_ld, mul, add_p, 1);
        g.a[0].first_base = h0;
    }
    g.Bt = ts->W_(l.iwr); g.bias = nullptr; g.M = B; g.N = 4 * W; g.Ktot = l.kr;
    g.zinit = mkslot(l.Z.as<float>(), 4 * W, (long long)B * 4 * W, mul, add_t);
    g.out = mkslot(l.hs, (int)l.hs_ld, (long long)B * l.hs_ld, mul, add_t);
    g.c_in = mkseg(l.Cs.as<float>(), W, W, 0, nullptr, (long long)B * W, mul, add_p, 1);
    g.c_in.first_base = c0;
    g.c_out = mkslot(l.Cs.as<float>(), W, (long long)B * W, mul, add_t);
    g.gates_out = mkslot(l.Gt.as<float>(), 4 * W, (long long)B * 4 * W, mul, add_t);
    g.step_imm = k; g.step_ptr = nullptr; g.kgroups = 2;
    return g;
}

static int time_of(const TLayer& l, int k) { return l.reverse ? l.len - 1 - k : k; }

// Z = x . Wx^T + b for every time step (one GEMM)
static void layer_input_gemm(casv_model* m, TLayer& l, const float* x, long long ldx) {
    TrainState* ts = m->train;
    GemmArgs g = plain_gemm(x, ldx, l.len * l.rows, l.kx, ts->W_(l.iwx), 4 * m->W, ts->W_(l.ib), l.Z.as<float>(), 4 * m->W);
    run_plain(m, g);
}

// weight gradients of one layer from dZ (in l.Z), its inputs x and its recurrent-side inputs rec [len*B][kr]: both
// contractions run over the rows = time x batch, on the operands as they lie
static int layer_weight_grads(casv_model* m, TLayer& l, const float* x, long long ldx, const float* rec, long long ldrec) {
    TrainState* ts = m->train;
    const int W = m->W;
    const long long rows = (long long)l.len * ts->B;
    if (ts->tens[l.iwx].frozen) return 0;
    // (the bias gradient = column sums of dZ rides in the first of the two launches)
    run_gemm_tn(m, l.Z.as<float>(), 4 * W, 4 * W, 4 * W, x, ldx, l.kx, rows, ts->G_(l.iwx), l.kx, ts->G_(l.ib));
    run_gemm_tn(m, l.Z.as<float>(), 4 * W, 4 * W, 4 * W, rec, ldrec, l.kr, rows, ts->G_(l.iwr), l.kr);
    return 0;
}

// Backward of plain LSTM layers.  dOut (+mask) = gradient w.r.t. the layer's output sequence; dh_fin/dc_fin w.r.t. its
// final state; h0/c0 its initial state (nullptr = zero).  Leaves dL/dh0 in dRec slot(first step) and dL/dc0 in dc.
struct LayerBwd {
    TLayer* l;
    const float* dOut; long long ld_out; const float* mask;
    const float* dh_fin; const float* dc_fin; const float* h0; const float* c0; float* dc;
    const float* x; long long ldx; float* dX; long long ld_dx; int dx_accumulate;
};

// pointwise part of processing index k (gate derivatives -> dZ)
static LstmBwdArgs layer_backward_pointwise(casv_model* m, const LayerBwd& a, int k) {
    TrainState* ts = m->train;
    TLayer& l = *a.l;
    const int W = m->W, B = ts->B;
    const int t = time_of(l, k);
    LstmBwdArgs p{};
    p.a = a.dOut ? a.dOut + (long long)t * B * a.ld_out : nullptr; p.lda = a.ld_out; p.mask_a = a.mask;
    if (k < l.len - 1) { p.b = l.dRec.as<float>() + (long long)time_of(l, k + 1) * B * W; p.ldb = W; }
    else if (a.dh_fin) { p.b = a.dh_fin; p.ldb = W; }
    p.gates = l.Gt.as<float>() + (long long)t * B * 4 * W;
    p.cell = l.Cs.as<float>() + (long long)t * B * W;
    if (k > 0) { p.c_prev = l.Cs.as<float>() + (long long)time_of(l, k - 1) * B * W; p.ld_cprev = W; }
    else { p.c_prev = a.c0; p.ld_cprev = W; }
    p.dc = a.dc; p.dz = l.Z.as<float>() + (long long)t * B * 4 * W; p.rows = B; p.W = W;
    return p;
}
// ... and the data GEMM that carries dZ to the previous step
static GemmArgs layer_backward_gemm(casv_model* m, const LayerBwd& a, int k) {
    TrainState* ts = m->train;
    TLayer& l = *a.l;
    const int W = m->W, B = ts->B;
    const int t = time_of(l, k);
    GemmArgs g = plain_gemm(l.Z.as<float>() + (long long)t * B * 4 * W, 4 * W, B, 4 * W, l.wrT.as<float>(), l.kr, nullptr,
                            l.dRec.as<float>() + (long long)t * B * W, W);
    g.out_zeroed = 1;           // casv_train_step clears dRec once per step
    return g;
}

static int layer_backward_finish(casv_model* m, const LayerBwd& a) {
    TrainState* ts = m->train;
    TLayer& l = *a.l;
    const int W = m->W, B = ts->B;
    const long long rows = (long long)l.len * B;
    if (a.dX) {
        GemmArgs g = plain_gemm(l.Z.as<float>(), 4 * W, (int)rows, 4 * W, l.wxT.as<float>(), l.kx, nullptr, a.dX, a.ld_dx, a.dx_accumulate);
        run_plain(m, g);
    }
    // The recurrent-side input of a step is the h of the previously processed step (h0 / zero at the first): the layer's own
    // outputs, one time step apart from dZ -- contracted as they lie (gemm_tn takes a row offset and a row stride; the first step's
    // B rows against h0 as a launch of their own), not copied into a shifted image first (105 MB per layer at configs[3]).
    if (ts->tens[l.iwx].frozen) return 0;
    const float* dZ = l.Z.as<float>();
    // (the bias gradient = column sums of dZ rides in the launch over the inputs)
    run_gemm_tn(m, dZ, 4 * W, 4 * W, 4 * W, a.x, a.ldx, l.kx, rows, ts->G_(l.iwx), l.kx, ts->G_(l.ib));
    const long long rest = (long long)(l.len - 1) * B;         // rows whose previous step is a row of hs
    if (rest > 0) {
        // forward layer: dZ[1..] with H[0..len-2]; reversed layer: dZ[0..len-2] with H[1..]
        const float* dz = dZ + (l.reverse ? 0 : (long long)B * 4 * W);
        const float* hp = l.hs + (l.reverse ? (long long)B * l.hs_ld : 0);
        run_gemm_tn(m, dz, 4 * W, 4 * W, 4 * W, hp, l.hs_ld, W, rest, ts->G_(l.iwr), l.kr);
    }
    if (a.h0) run_gemm_tn(m, dZ + (long long)time_of(l, 0) * B * 4 * W, 4 * W, 4 * W, 4 * W, a.h0, W, W, B, ts->G_(l.iwr), l.kr);
    return 0;
}

// Up to two independent layers walk their sequences backwards in lockstep: one pointwise launch each and ONE data-GEMM
// launch per step for both (the per-step launches are latency-bound, so pairing them is nearly free).
static int layers_backward(casv_model* m, const LayerBwd* a, int count) {
    TrainState* ts = m->train;
    const int W = m->W, B = ts->B;
    int maxlen = 0;
    for (int j = 0; j < count; ++j) {
        if (a[j].dc_fin) HIPCHK(hipMemcpyAsync(a[j].dc, a[j].dc_fin, (size_t)B * W * 4, hipMemcpyDeviceToDevice, m->stream));
        else HIPCHK(hipMemsetAsync(a[j].dc, 0, (size_t)B * W * 4, m->stream));
        maxlen = std::max(maxlen, a[j].l->len);
    }
    bool persistent = false, plain = true;
    double flops = 0;
    for (int j = 0; j < count; ++j) { plain = plain && a[j].l->kr == W; flops += 2.0 * B * 4.0 * W * W * a[j].l->len; }
    if (int rc = persist_launch(m, persist_site(TRAIN_REC_BWD, {W, m->C, B, maxlen, count}, plain), flops, &persistent, [&](const TrainLaunch& plan, unsigned* counters) {
            RecBwdArgs ra{};
            ra.njobs = count; ra.B = B; ra.W = W; ra.counters = counters;
            for (int j = 0; j < count; ++j) {
                TLayer& l = *a[j].l;
                ra.job[j] = RecBwdJob{l.wrT.as<float>(), a[j].dOut, a[j].ld_out, a[j].mask, a[j].dh_fin, a[j].dc_fin, l.Gt.as<float>(), l.Cs.as<float>(), a[j].c0,
                                      l.Z.as<float>(), l.dRec.as<float>(), a[j].dc, l.len, l.reverse ? 1 : 0};
            }
            launch_train_recurrence_bwd(ra, plan.grid, m->stream);
            return 0;
        })) return rc;
    if (persistent) {
    } else if (m->fused_backward && !m->deterministic) {
        // one launch per step for both layers: the cells' backward inside the data GEMM (gemm_bwd.hip); dL/dc ping-pongs
        float* dcb[2][2];
        int done[2] = {0, 0};
        for (int j = 0; j < count; ++j) { dcb[j][0] = a[j].dc; dcb[j][1] = ts->dcalt.as<float>() + (size_t)j * B * W; }
        for (int i = 0; i < maxlen; ++i) {
            BwdStepBatch fb{};
            double flops = 0, bytes = 0;
            for (int j = 0; j < count; ++j) {
                const int k = a[j].l->len - 1 - i;
                if (k < 0) continue;
                BwdStepJob& q = fb.j[fb.count++];
                q.p = layer_backward_pointwise(m, a[j], k);
                q.dc_in = dcb[j][done[j] & 1]; q.p.dc = dcb[j][(done[j] + 1) & 1];
                ++done[j];
                const GemmArgs g = layer_backward_gemm(m, a[j], k);
                q.Bt = g.Bt; q.out = g.out.base; q.ld_out = g.out.ld; q.N = g.N;
                flops += 2.0 * B * (double)g.N * 4.0 * W; bytes += 4.0 * ((double)B * 4 * W + (double)g.N * 4 * W + (double)B * g.N);
            }
            hipEvent_t ev{};
            m->prof_begin(PC_GEMM, flops, bytes, ev);
            launch_lstm_bwd_gemm(fb, m->stream);
            m->prof_end(PC_GEMM, ev);
        }
        for (int j = 0; j < count; ++j)
            if (done[j] & 1) HIPCHK(hipMemcpyAsync(a[j].dc, dcb[j][1], (size_t)B * W * 4, hipMemcpyDeviceToDevice, m->stream));
    } else
    for (int i = 0; i < maxlen; ++i) {
        GemmBatch b{};
        LstmBwdBatch pw{};
        for (int j = 0; j < count; ++j) {
            const int k = a[j].l->len - 1 - i;
            if (k < 0) continue;
            pw.a[pw.count++] = layer_backward_pointwise(m, a[j], k);
            b.g[b.count++] = layer_backward_gemm(m, a[j], k);
        }
        launch_lstm_bwd_batch(pw, m->stream);
        run_gemm_batch(m, EPI_PLAIN, b);
    }
    for (int j = 0; j < count; ++j)
        if (int rc = layer_backward_finish(m, a[j])) return rc;
    return 0;
}

// Forward recurrence of up to two independent plain layers: ONE persistent launch (train_persist.hip) where the shape has
// one and the device is ours, else one launch per step for both (the two are interchangeable bit for bit).  Each layer walks its
// own rows (TLayer.rows): in a candidates call the encoder's job has Be of them beside the decoder's B -- the persistent launch
// keeps B's grid and counters (RecJob.rows), the per-step launch's jobs carry their own M.
// om / om_ld / omask: the layer's outputs once more, times the next layer's per-unit dropout mask (nullptr: times one) -- written by
// the persistent recurrence itself; *masked tells the caller whether it was (the per-step launches leave it to launch_mul_mask).
struct LayerFwd { TLayer* l; const float* h0; const float* c0; float* om = nullptr; long long om_ld = 0; const float* omask = nullptr; };
static int layers_forward(casv_model* m, const LayerFwd* a, int count, bool* masked = nullptr) {
    if (masked) *masked = false;
    TrainState* ts = m->train;
    const int W = m->W, B = ts->B;
    int maxlen = 0;
    double flops = 0;
    for (int j = 0; j < count; ++j) { maxlen = std::max(maxlen, a[j].l->len); flops += 2.0 * a[j].l->rows * 4.0 * W * W * a[j].l->len; }
    bool persistent = false;
    if (int rc = persist_launch(m, persist_site(TRAIN_REC, {W, m->C, B, maxlen, count}), flops, &persistent, [&](const TrainLaunch& plan, unsigned* counters) {
            RecArgs ra{};
            ra.njobs = count; ra.B = B; ra.W = W; ra.counters = counters;
            ra.fault = m->persist_mode == 2;       // (test of the give-up path)
            for (int j = 0; j < count; ++j) {
                TLayer& l = *a[j].l;
                ra.job[j] = RecJob{ts->W_(l.iwr), l.Z.as<float>(), l.hs, l.hs_ld, l.Cs.as<float>(), l.Gt.as<float>(), a[j].h0, a[j].c0, l.len,
                                   l.reverse ? 1 : 0, masked ? a[j].om : nullptr, a[j].om_ld, a[j].omask, l.kr == W ? l.dRec.as<float>() : nullptr,        // (a scoring state has no dRec: nullptr, nothing to clear)
                                   l.rows == B ? 0 : l.rows};                           // (the encoder's job of a candidates call: Be < B rows)
                l.drec_cleared = l.kr == W;
            }
            launch_train_recurrence(ra, plan.grid, m->stream);
            return 0;
        })) return rc;
    if (persistent) {
        if (masked) *masked = true;
        return 0;
    }
    for (int k = 0; k < maxlen; ++k) {
        GemmBatch b{};
        for (int j = 0; j < count; ++j)
            if (k < a[j].l->len) b.g[b.count++] = layer_step_job(m, *a[j].l, k, a[j].h0, a[j].c0, nullptr);
        run_gemm_batch(m, EPI_LSTM, b);
    }
    return 0;
}

// Phase 1 leaves every buffer of the session at least as large as this step's shapes ask, every layer's len / hs / hs_ld, and the
// view's pointers into the state buffers (read behind the calls that may have moved them).
int plan_buffers(Step& s) {
    casv_model* m = s.m; TrainState* ts = s.ts;
    const int B = s.B, Be = s.Be, T = s.T, U = s.U, A = s.A, W = s.W, V = s.V, Vp = s.Vp, C = s.C, D = s.D;
    const long long TB = s.TB, UB = s.UB;
    const bool deep = s.deep;
    const bool bwd = !ts->forward_only;     // (a scoring state holds no backward buffer: BWD(...) allocates in a session only)
#define ENS(buf, bytes) if (int rc_ = (buf).ensure(bytes)) return rc_;
#define BWD(buf, bytes) if (bwd) ENS(buf, bytes)
    ENS(ts->e_idx, TB * A * 4) ENS(ts->e_val, TB * A * 4) ENS(ts->d_in, UB * 4) ENS(ts->d_out, UB * 4) ENS(ts->d_w, UB * 4)
    ENS(ts->m_enc, (size_t)std::max(D + 1, 2 * D) * W * 4) ENS(ts->m_dec, (size_t)D * W * 4) ENS(ts->m_cell, (size_t)B * (W + C) * 4)
    ENS(ts->X0, TB * W * 4) ENS(ts->H1, TB * 2 * W * 4) ENS(ts->u, TB * W * 4) ENS(ts->Y0, UB * W * 4) ENS(ts->Ym, UB * W * 4)
    ENS(ts->WQ, UB * W * 4) ENS(ts->Ast, (size_t)(U + 1) * B * T * 4) ENS(ts->WIN, UB * 4)
    ENS(ts->RecIn, UB * (C + W) * 4) ENS(ts->logits, UB * Vp * 4)
    BWD(ts->dG, UB * W * 4) BWD(ts->d_enc, TB * C * 4) BWD(ts->du, TB * W * 4) BWD(ts->DWQ, UB * W * 4) BWD(ts->DSrows, UB * 16 * 4) BWD(ts->dhatt, UB * W * 4)
    BWD(ts->dfin, (size_t)2 * D * B * W * 4) BWD(ts->dcbuf, (size_t)B * W * 4)
    BWD(ts->dX0, TB * W * 4) BWD(ts->dXtop, UB * W * 4) BWD(ts->dXl, TB * 2 * W * 4) BWD(ts->dYl, UB * W * 4) BWD(ts->dOin, TB * 2 * W * 4)
    BWD(ts->dcbuf2, (size_t)B * W * 4) BWD(ts->dvaP, (size_t)B * W * 4) BWD(ts->dbvP, (size_t)B * 4)
    for (auto& l : ts->layers) {
        const bool enc = l.encoder;
        l.len = enc ? T : U; l.rows = enc ? Be : B;
        const long long rows = (long long)l.len * l.rows;
        ENS(l.Cs, rows * W * 4) ENS(l.Gt, rows * 4 * W * 4) ENS(l.Z, rows * 4 * W * 4) BWD(l.dRec, rows * l.kr * 4)
        const bool first = &l < &ts->layers[2];         // (layer 1's two directions share H1)
        if (first) { l.hs = ts->H1.as<float>() + l.dir * W; l.hs_ld = 2 * W; }
        else if (deep && enc && l.dir == 0) { ENS(l.Hown, rows * 2 * W * 4) l.hs = l.Hown.as<float>(); l.hs_ld = 2 * W; }
        else if (deep && enc) { l.hs = (&l - 1)->hs + W; l.hs_ld = 2 * W; }        // (a backward direction: the second half of its forward partner's rows)
        else { ENS(l.Hown, rows * W * 4) l.hs = l.Hown.as<float>(); l.hs_ld = W; }
    }
    ENS(ts->rec_cnt, TRAIN_LAUNCH_CAP * train_slot_bytes(B)) BWD(ts->dcalt, (size_t)2 * B * W * 4)
    if (s.det) {
        ENS(ts->sum_parts, (size_t)std::max(MULTI_MAX * 64, (W + 63) / 64 + V) * 8)
        ENS(ts->seg_enc_off, (size_t)(V + 1) * 4) ENS(ts->seg_enc_pos, (size_t)TB * A * 4) ENS(ts->seg_dec_off, (size_t)(V + 1) * 4) ENS(ts->seg_dec_pos, (size_t)UB * 4)
    }
    if (s.bridged) { ENS(ts->hbr, (size_t)D * Be * W * 4) ENS(ts->cbr, (size_t)D * Be * W * 4) ENS(ts->brtmp, (size_t)Be * W * 4) }
    if (s.K > 0) { ENS(ts->d_sidx, UB * s.K * 4) ENS(ts->d_sq, UB * s.K * 4) }
    if (s.RN > 0) {
        ENS(ts->r_cost, (size_t)B * 4) ENS(ts->r_coef, (size_t)B * 4) ENS(ts->r_q, (size_t)B * 8) ENS(ts->r_risk, (size_t)(B / s.RN) * 8)
        ENS(ts->r_parts, (size_t)(B / s.RN) * 8) ENS(ts->s_logp, UB * 4) ENS(ts->s_best, UB * 4) ENS(ts->s_rank, UB * 4)
    }
    if (s.sched) { ENS(ts->d_gold, UB * 4) ENS(ts->d_mix, (size_t)s.sched->passes * UB * 4) }
    if (s.N > 1) { ENS(ts->h0rep, (size_t)D * B * W * 4) ENS(ts->c0rep, (size_t)D * B * W * 4) }
    if (s.residual && D >= 2) ENS(ts->Ytop, UB * W * 4)
    for (int n = 1; n <= D; ++n) ENS(ts->O[n], TB * ((n == 1 || deep) ? 2 * W : W) * 4)
    for (int n = 2; n <= D && deep; ++n) ENS(ts->XD[n], TB * 2 * W * 4)
    for (int n = 1; n < D; ++n) ENS(ts->DO[n], UB * W * 4)
    ENS(m->hfin, (size_t)D * B * W * 4) ENS(m->cfin, (size_t)(D + 1) * B * W * 4)       // (shared with the inference session)
#undef BWD
#undef ENS
    s.hfin = m->hfin.as<float>(); s.cfin = m->cfin.as<float>();
    // bridge_dense (seq2seq.py:299-301): the decoder starts from tanh(state . K + b) of every encoder layer's final h and c
    s.h0base = s.bridged ? ts->hbr.as<float>() : s.hfin; s.c0base = s.bridged ? ts->cbr.as<float>() : s.cfin;
    if (s.N > 1) { s.h0base = ts->h0rep.as<float>(); s.c0base = ts->c0rep.as<float>(); }     // (filled layer by layer: repeat_states)
    s.dfin = ts->dfin.as<float>();
    s.parts = s.det ? ts->sum_parts.as<double>() : nullptr;
    return 0;
}

// per-character segments of an index array [B][L][A_], positions in (t, b, k) order within a character (counting sort on the host)
void char_segments(const int32_t* idx, int B, int L, int A_, int V, std::vector<int>& off, std::vector<int>& pos) {
    off.assign(V + 2, 0);
    for (long long q = 0; q < (long long)B * L * A_; ++q) if (idx[q] >= 0 && idx[q] < V) ++off[idx[q] + 2];
    for (int v = 0; v < V; ++v) off[v + 2] += off[v + 1];
    pos.resize(std::max<size_t>(1, off[V + 1]));
    for (int t = 0; t < L; ++t)
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < A_; ++k) {
                const long long q = ((long long)b * L + t) * A_ + k;
                if (idx[q] >= 0 && idx[q] < V) pos[off[idx[q] + 1]++] = (int)q;
            }
    off.pop_back();             // off[v] = first position of character v, off[V] = count
}

// Phase 2 leaves the batch, the masks and (deterministic) the characters' segments on the device, the step's sums, hand-off counters
// and (training) gradients cleared, and the session's per-step state reset.
int stage_inputs(Step& s) {
    TrainState* ts = s.ts; hipStream_t st = s.st;
    const int B = s.B, T = s.T, U = s.U, A = s.A, W = s.W, V = s.V, C = s.C, D = s.D;
    const long long TB = s.TB, UB = s.UB;
    HIPCHK(hipMemcpyAsync(ts->e_idx.p, s.enc_idx, TB * A * 4, hipMemcpyHostToDevice, st));
    if (s.enc_val) HIPCHK(hipMemcpyAsync(ts->e_val.p, s.enc_val, TB * A * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ts->d_in.p, s.dec_in, UB * 4, hipMemcpyHostToDevice, st));
    if (s.sched) HIPCHK(hipMemcpyAsync(ts->d_gold.p, s.dec_in, UB * 4, hipMemcpyHostToDevice, st));
    if (s.K > 0) {
        HIPCHK(hipMemcpyAsync(ts->d_sidx.p, s.soft_idx, UB * s.K * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ts->d_sq.p, s.soft_q, UB * s.K * 4, hipMemcpyHostToDevice, st));
    } else HIPCHK(hipMemcpyAsync(ts->d_out.p, s.dec_out, UB * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ts->d_w.p, s.weights, UB * 4, hipMemcpyHostToDevice, st));
    if (s.RN > 0) HIPCHK(hipMemcpyAsync(ts->r_cost.p, s.cost, (size_t)B * 4, hipMemcpyHostToDevice, st));
    if (s.det) {
        char_segments(s.enc_idx, s.Be, T, A, V, ts->h_seg_enc_off, ts->h_seg_enc_pos);
        char_segments(s.dec_in, B, U, 1, V, ts->h_seg_dec_off, ts->h_seg_dec_pos);
        HIPCHK(hipMemcpyAsync(ts->seg_enc_off.p, ts->h_seg_enc_off.data(), (size_t)(V + 1) * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ts->seg_enc_pos.p, ts->h_seg_enc_pos.data(), ts->h_seg_enc_pos.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ts->seg_dec_off.p, ts->h_seg_dec_off.data(), (size_t)(V + 1) * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ts->seg_dec_pos.p, ts->h_seg_dec_pos.data(), ts->h_seg_dec_pos.size() * 4, hipMemcpyHostToDevice, st));
    }
    s.menc = s.mdec = s.mcell = nullptr;
    if (s.mask_enc) { HIPCHK(hipMemcpyAsync(ts->m_enc.p, s.mask_enc, (size_t)(s.deep ? 2 * D : D + 1) * W * 4, hipMemcpyHostToDevice, st)); s.menc = ts->m_enc.as<float>(); }
    if (s.mask_dec && D > 1) { HIPCHK(hipMemcpyAsync(ts->m_dec.p, s.mask_dec, (size_t)(D - 1) * W * 4, hipMemcpyHostToDevice, st)); s.mdec = ts->m_dec.as<float>(); }
    if (s.mask_cell) { HIPCHK(hipMemcpyAsync(ts->m_cell.p, s.mask_cell, (size_t)B * (W + C) * 4, hipMemcpyHostToDevice, st)); s.mcell = ts->m_cell.as<float>(); }
    long cnt = 0;
    for (long long i = 0; i < UB; ++i) cnt += s.weights[i] != 0.f;
    s.inv_count = 1.0f / (float)std::max(cnt, 1L);
    HIPCHK(hipMemsetAsync(ts->loss.p, 0, 16, st));
    HIPCHK(hipMemsetAsync(ts->normsq.p, 0, 16, st));
    HIPCHK(hipMemsetAsync(ts->rec_cnt.p, 0, TRAIN_LAUNCH_CAP * train_slot_bytes(B), st));
    ts->plan = TrainStepPlan{}; ts->rec_checked = 0; ts->split_launch = -1; ts->tn_ws_rc = 0;
    for (auto& l : ts->layers) l.drec_cleared = false;
    if (ts->rec_skip > 0) --ts->rec_skip;
    if (s.training) for (auto& t : ts->tens) HIPCHK(hipMemsetAsync(t.g.p, 0, t.n * 4, st));
    return 0;
}

// bridge_dense forward of encoder layer n (1-based): hfin / cfin slot n - 1 -> hbr / cbr slot n - 1
static void bridge_forward(Step& s, int n) {
    if (!s.bridged) return;
    casv_model* m = s.m; TrainState* ts = s.ts;
    const int B = s.Be, W = s.W;
    for (int s_ = 0; s_ < 2; ++s_) {
        const TrainState::Bridge& br = ts->bridge[2 * (n - 1) + s_];
        const float* src = (s_ ? s.cfin : s.hfin) + (size_t)(n - 1) * B * W;
        float* dst = (s_ ? ts->cbr.as<float>() : ts->hbr.as<float>()) + (size_t)(n - 1) * B * W;
        GemmArgs g = plain_gemm(src, W, B, W, ts->W_(br.ikt), W, ts->W_(br.ib), ts->brtmp.as<float>(), W);
        g.ksplit = 0; g.kgroups = 0;            // (one k-ordered chain per element, no atomics into an uncleared buffer)
        run_gemm(m, EPI_PLAIN, g);
        launch_tanh(ts->brtmp.as<float>(), dst, (long long)B * W, s.st);
    }
}

// N > 1: the decoder's initial states of layer n (1-based) = encoder layer n's final (bridged) states, every source's row once per
// candidate -- right behind that layer's final-state copy / bridge, ahead of the launch that walks decoder layer n
static void repeat_states(Step& s, int n) {
    if (s.N == 1) return;
    TrainState* ts = s.ts;
    const size_t src = (size_t)(n - 1) * s.Be * s.W, dst = (size_t)(n - 1) * s.B * s.W;
    launch_repeat_rows((s.bridged ? ts->hbr.as<float>() : s.hfin) + src, ts->h0rep.as<float>() + dst, s.Be, s.N, s.W, s.st);
    launch_repeat_rows((s.bridged ? ts->cbr.as<float>() : s.cfin) + src, ts->c0rep.as<float>() + dst, s.Be, s.N, s.W, s.st);
}

// Decoder layer k (1 .. D-1, below the cell) alone in its launch, on the input sequence y [U*B][W]: its outputs, cell states and gates,
// and the cell's / the next layer's input DO[k] -- the outputs (residual_connections, k >= 2: plus y) times the next dropout mask.
int decoder_layer_alone(Step& s, int k, const float* y) {
    casv_model* m = s.m; TrainState* ts = s.ts;
    const int W = s.W;
    TLayer& ld = s.dec_layer(k);
    layer_input_gemm(m, ld, y, W);
    const bool res = s.residual && k >= 2;
    bool masked = false;
    const LayerFwd f[1] = {{&ld, s.dec_h0(k), s.dec_c0(k), res ? nullptr : ts->DO[k].as<float>(), W, s.mdec_n(k)}};
    if (int rc = layers_forward(m, f, 1, &masked)) return rc;
    if (res) launch_add_mul_mask(ld.hs, W, y, W, s.mdec_n(k), ts->DO[k].as<float>(), W, s.UB, W, s.st);
    else if (!masked) launch_mul_mask(ld.hs, W, s.mdec_n(k), ts->DO[k].as<float>(), W, s.UB, W, s.st);
    return 0;
}

// Phase 3 leaves every encoder layer's and every decoder layer's below the cell outputs, cell states and gates, the masked outputs
// O[n] / DO[n], the final states (and the bridged ones), the cell's input sequence s.y, the attended sequence s.enc_out and its
// projection u.
int forward_layers(Step& s) {
    casv_model* m = s.m; TrainState* ts = s.ts; hipStream_t st = s.st;
    const int B = s.B, Be = s.Be, T = s.T, U = s.U, A = s.A, W = s.W, V = s.V, C = s.C, D = s.D;      // (Be: the encoder's rows, B: the decoder's)
    const long long TB = s.TB, UB = s.UB;
    const bool deep = s.deep, residual = s.residual;
    float* hfin = s.hfin; float* cfin = s.cfin;
    TLayer* Lfw = &ts->layers[0]; TLayer* Lbw = &ts->layers[1];
    launch_embed_tm(ts->W_(ts->iE), ts->e_idx.as<int>(), s.enc_val ? ts->e_val.as<float>() : nullptr, ts->X0.as<float>(), Be, T, A, V, W, st);
    layer_input_gemm(m, *Lfw, ts->X0.as<float>(), W);
    layer_input_gemm(m, *Lbw, ts->X0.as<float>(), W);
    bool masked1 = false;
    {
        const LayerFwd f[2] = {{Lfw, nullptr, nullptr, ts->O[1].as<float>(), 2 * W, s.menc_n(1)},
                               {Lbw, nullptr, nullptr, ts->O[1].as<float>() + W, 2 * W, s.menc_n(1) ? s.menc_n(1) + W : nullptr}};
        if (int rc = layers_forward(m, f, 2, &masked1)) return rc;
    }
    // final states handed to the decoder: layer 1 = backward direction after t = 0 (seq2seq.py:280)
    HIPCHK(hipMemcpy2DAsync(hfin, (size_t)W * 4, Lbw->hs, (size_t)2 * W * 4, (size_t)W * 4, Be, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(cfin, Lbw->Cs.p, (size_t)Be * W * 4, hipMemcpyDeviceToDevice, st));
    bridge_forward(s, 1);
    repeat_states(s, 1);
    if (!masked1) launch_mul_mask(ts->H1.as<float>(), 2 * W, s.menc_n(1), ts->O[1].as<float>(), 2 * W, TB, 2 * W, st);
    launch_embed_tm(ts->W_(ts->iE), ts->d_in.as<int>(), nullptr, ts->Y0.as<float>(), B, U, 1, V, W, st);
    // Encoder layer n and decoder layer n-1 depend only on encoder layer n-1 / decoder layer n-2, so the two
    // recurrences advance in lockstep, one launch per step for both.
    const float* y = ts->Y0.as<float>();
    // deep_bidirectional_encoder (seq2seq.py:246-281): every encoder layer n >= 2 is a BiLSTM on the cross sum of the (dropped-out) layer
    // below; its two directions are the pair of a launch, the decoder layer n - 1 walks alone
    for (int n = 2; n <= D && deep; ++n) {
        TLayer& lf = s.enc_dir(n, 0); TLayer& lb = s.enc_dir(n, 1);
        launch_cross_sum(ts->O[n - 1].as<float>(), ts->XD[n].as<float>(), TB * 2 * W, st);
        layer_input_gemm(m, lf, ts->XD[n].as<float>(), 2 * W);
        layer_input_gemm(m, lb, ts->XD[n].as<float>(), 2 * W);
        bool maskede = false;
        {
            const LayerFwd f[2] = {{&lf, nullptr, nullptr, ts->O[n].as<float>(), 2 * W, s.menc_n(n)},
                                   {&lb, nullptr, nullptr, ts->O[n].as<float>() + W, 2 * W, s.menc_n(n) ? s.menc_n(n) + W : nullptr}};
            if (int rc = layers_forward(m, f, 2, &maskede)) return rc;
        }
        HIPCHK(hipMemcpy2DAsync(hfin + (size_t)(n - 1) * Be * W, (size_t)W * 4, lb.hs, (size_t)2 * W * 4, (size_t)W * 4, Be, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(cfin + (size_t)(n - 1) * Be * W, lb.Cs.p, (size_t)Be * W * 4, hipMemcpyDeviceToDevice, st));
        bridge_forward(s, n);
        repeat_states(s, n);
        if (!maskede) launch_mul_mask(lf.hs, 2 * W, s.menc_n(n), ts->O[n].as<float>(), 2 * W, TB, 2 * W, st);
        if (int rc = decoder_layer_alone(s, n - 1, y)) return rc;
        y = ts->DO[n - 1].as<float>();
    }
    for (int n = 2; n <= D && !deep; ++n) {
        TLayer& le = s.enc_layer(n);
        TLayer& ld = s.dec_layer(n - 1);
        layer_input_gemm(m, le, ts->O[n - 1].as<float>(), le.kx);
        layer_input_gemm(m, ld, y, W);
        // residual_connections: encoder layer n >= 3 / decoder layer n - 1 >= 2 hand on LSTM output + input sequence (seq2seq.py:284-291,
        // 359-360) -- the sum and the next layer's dropout mask in one pass behind the recurrences (which then write no masked copy)
        const bool res_n = residual && n >= 3;
        bool maskedn = false;
        {
            const LayerFwd f[2] = {{&le, nullptr, nullptr, res_n ? nullptr : ts->O[n].as<float>(), W, s.menc_n(n)},
                                   {&ld, s.dec_h0(n - 1), s.dec_c0(n - 1), res_n ? nullptr : ts->DO[n - 1].as<float>(), W, s.mdec_n(n - 1)}};
            if (int rc = layers_forward(m, f, 2, &maskedn)) return rc;
        }
        HIPCHK(hipMemcpyAsync(hfin + (size_t)(n - 1) * Be * W, le.hs + (long long)(T - 1) * Be * W, (size_t)Be * W * 4, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(cfin + (size_t)(n - 1) * Be * W, le.Cs.as<float>() + (long long)(T - 1) * Be * W, (size_t)Be * W * 4, hipMemcpyDeviceToDevice, st));
        bridge_forward(s, n);
        repeat_states(s, n);
        if (res_n) {
            launch_add_mul_mask(le.hs, W, ts->O[n - 1].as<float>(), W, s.menc_n(n), ts->O[n].as<float>(), W, TB, W, st);
            launch_add_mul_mask(ld.hs, W, y, W, s.mdec_n(n - 1), ts->DO[n - 1].as<float>(), W, UB, W, st);
        } else if (!maskedn) {
            launch_mul_mask(le.hs, W, s.menc_n(n), ts->O[n].as<float>(), W, TB, W, st);
            launch_mul_mask(ld.hs, W, s.mdec_n(n - 1), ts->DO[n - 1].as<float>(), W, UB, W, st);
        }
        y = ts->DO[n - 1].as<float>();
    }
    s.y = y;
    s.enc_out = ts->O[D].as<float>();
    { GemmArgs g = plain_gemm(s.enc_out, C, (int)TB, C, ts->W_(ts->iUT), W, nullptr, ts->u.as<float>(), W); run_plain(m, g); }
    return 0;
}

// Phase 4 leaves the attention cell's outputs, cell states and gates, its input rows RecIn, the queries WQ, the attention rows Ast
// and the windows WIN of every step.
int forward_cell(Step& s) {
    casv_model* m = s.m; TrainState* ts = s.ts; hipStream_t st = s.st;
    const int B = s.B, T = s.T, U = s.U, W = s.W, C = s.C, D = s.D;
    const long long UB = s.UB;
    const float* mcell = s.mcell;
    TLayer& top = s.top();
    launch_mul_rowmask(s.y, W, mcell, W + C, ts->Ym.as<float>(), W, UB, B, W, st);
    layer_input_gemm(m, top, ts->Ym.as<float>(), W);
    const float* h0t = s.dec_h0(D); const float* c0t = s.dec_c0(D);
    HIPCHK(hipMemsetAsync(ts->Ast.p, 0, (size_t)B * T * 4, st));
    // The cell's input rows [ctx * mask | h(t-1)] (LSTMCell(dropout) masks the cell input [y | ctx] per sample, seq2seq.py:345; the y
    // part is masked where it is precomputed) are filled where their parts are produced: the attention rows write the masked
    // context straight into them, the cell of the step before stores its h a second time.
    HIPCHK(hipMemcpy2DAsync(ts->RecIn.as<float>() + C, (size_t)(C + W) * 4, h0t, (size_t)W * 4, (size_t)W * 4, B, hipMemcpyDeviceToDevice, st));
    AttnArgs att{};         // what every step's attention rows share
    att.u = ts->u.as<float>(); att.enc = s.enc_out; att.va = ts->W_(ts->iva); att.bv = ts->W_(ts->ibv);
    att.a_base = ts->Ast.as<float>(); att.prev = nullptr; att.line = nullptr; att.rows_per_line = s.N;     // (decoder row r attends source r / N)
    att.ctx_ld = C + W; att.ctx_mask = mcell ? mcell + W : nullptr; att.ctx_mask_ld = W + C;
    att.R = B; att.T = T; att.W = W; att.C = C; att.window = m->cfg.window_width;
    att.apos = nullptr; att.amax1 = nullptr; att.nrows = nullptr;
    att.u_line = W; att.u_time = (long long)s.Be * W; att.enc_line = C; att.enc_time = (long long)s.Be * C;
    bool top_persistent = false;
    // ONE launch for the whole recurrence of the cell (train_persist_top.hip)
    if (int rc = persist_launch(m, persist_site(TRAIN_CELL, {W, C, B, U, 1}, top.hs_ld == W), 2.0 * B * U * ((double)4 * W * (C + W) + (double)W * W),
                                &top_persistent, [&](const TrainLaunch& plan, unsigned* counters) {
            TopRecArgs ra{};
            ra.Wr = ts->W_(top.iwr); ra.WaT = ts->W_(ts->iWaT); ra.bUW = ts->W_(ts->ibUW); ra.Z = top.Z.as<float>();
            ra.RecIn = ts->RecIn.as<float>(); ra.WQ = ts->WQ.as<float>(); ra.hs = top.hs; ra.Cs = top.Cs.as<float>(); ra.Gt = top.Gt.as<float>();
            ra.c0 = c0t; ra.WIN = ts->WIN.as<int>(); ra.att = att; ra.B = B; ra.U = U; ra.W = W; ra.C = C; ra.counters = counters;
            launch_train_attention_cell(ra, plan.grid, st);
            return 0;
        })) return rc;
    if (!top_persistent) HIPCHK(hipMemsetAsync(ts->WQ.p, 0, UB * W * 4, st));      // (the per-step launches' split-K partial sums land here; the persistent kernel stores its queries)
    for (int t = 0; t < U && !top_persistent; ++t) {
        const float* hprev = t == 0 ? h0t : top.hs + (long long)(t - 1) * B * W;
        float* wq = ts->WQ.as<float>() + (long long)t * B * W;
        { GemmArgs g = plain_gemm(hprev, W, B, W, ts->W_(ts->iWaT), W, ts->W_(ts->ibUW), wq, W); g.out_zeroed = 1; run_gemm(m, EPI_PLAIN, g); }
        AttnArgs a = att;
        float* rec = ts->RecIn.as<float>() + (long long)t * B * (C + W);
        a.wq = wq; a.ctx = rec; a.step_imm = t; a.step_ptr = nullptr;
        a.win_out = ts->WIN.as<int>() + (long long)t * B;
        launch_attention(a, st);
        GemmArgs g = layer_step_job(m, top, t, nullptr, c0t, ts->RecIn.as<float>());
        g.c_in.skip_first = 0;
        if (t + 1 < U) g.out2 = mkslot(rec + (long long)B * (C + W) + C, C + W);
        run_gemm(m, EPI_LSTM, g);
    }
    return 0;
}

// The tied output projection: leaves its input s.proj_in and the logits [U*B][Vp] (columns [V, Vp) are not written).
int projection(Step& s) {
    casv_model* m = s.m; TrainState* ts = s.ts; hipStream_t st = s.st;
    const int W = s.W, V = s.V, Vp = s.Vp;
    const long long UB = s.UB;
    TLayer& top = s.top();
    // (residual_connections: the projection reads the cell's outputs PLUS the cell's input sequence, seq2seq.py:359-360 at the top layer)
    s.proj_in = top.hs; s.proj_ld = W;
    if (s.res_top()) {
        launch_add_mul_mask(top.hs, top.hs_ld, s.y, W, nullptr, ts->Ytop.as<float>(), W, UB, W, st);
        s.proj_in = ts->Ytop.as<float>();
    }
    { GemmArgs g = plain_gemm(s.proj_in, s.proj_ld, (int)UB, W, ts->W_(ts->iE), V, nullptr, ts->logits.as<float>(), Vp); run_plain(m, g); }
    return 0;
}

// Phase 5 leaves the projection's input s.proj_in, the step's cross-entropy in ts->loss and (training) dL/dlogits in place of the logits.
static int loss_head(Step& s) {
    TrainState* ts = s.ts; hipStream_t st = s.st;
    const int B = s.B, U = s.U, V = s.V, Vp = s.Vp;
    if (int rc = projection(s)) return rc;
    hipEvent_t ev{};            // (casv_profile, class "softmax": the head reads the logits once and, training, writes them once)
    s.m->prof_begin(PC_SOFTMAX, 0.0, 4.0 * (double)s.UB * (V + (s.training ? Vp : 0)) + 8.0 * (double)s.UB * s.K + (s.RN > 0 ? 4.0 * (double)s.UB * V : 0.0), ev);
    if (s.RN > 0)
        launch_risk_head(ts->logits.as<float>(), ts->d_out.as<int>(), ts->d_w.as<float>(), ts->r_cost.as<float>(), B, U, V, Vp, s.RN, s.alpha,
                         s.inv_groups, ts->s_logp.as<float>(), ts->s_best.as<int>(), ts->s_rank.as<int>(), ts->r_coef.as<float>(),
                         ts->r_q.as<double>(), ts->r_risk.as<double>(), ts->r_parts.as<double>(), ts->loss.as<double>(), st);
    else if (s.K > 0)
        launch_soft_ce(ts->logits.as<float>(), ts->d_sidx.as<int>(), ts->d_sq.as<float>(), ts->d_w.as<float>(), B, U, V, Vp, s.K, s.inv_count,
                       ts->loss.as<double>(), s.training ? 1 : 0, st, s.parts);
    else
        launch_softmax_ce(ts->logits.as<float>(), ts->d_out.as<int>(), ts->d_w.as<float>(), B, U, V, Vp, s.inv_count, ts->loss.as<double>(),
                          s.training ? 1 : 0, st, s.parts);
    s.m->prof_end(PC_SOFTMAX, ev);
    return 0;
}

// Did every persistent recurrence so far run to its end?  (A launch gives up when its workgroups wait too long for each
// other -- a GPU shared with another process: handoff.h.)  Nothing has been updated yet: the caller starts over with per-step
// launches, and keeps to them for the next 16, 32, ... steps.  Asked after the forward pass and again in front of the update.
int recurrences_gave_up(casv_model* m, bool& any) {
    TrainState* ts = m->train; hipStream_t st = m->stream;
    any = false;
    if (ts->plan.launches == ts->rec_checked) return 0;
    unsigned gave_up[TRAIN_LAUNCH_CAP] = {0};
    for (int i = ts->rec_checked; i < ts->plan.launches; ++i)
        HIPCHK(hipMemcpyAsync(&gave_up[i], ts->rec_abort[i], 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = ts->rec_checked; i < ts->plan.launches; ++i) {
        any |= gave_up[i] != 0;
        if (gave_up[i] && i == ts->split_launch && !ts->split_off) {        // (the two launches were not resident together: one launch from now on)
            ts->split_off = true;
            fprintf(stderr, "cor_asv_ann_hip: the two launches of the attention cell's backward were not resident together (serialised "
                            "dispatch, or the GPU is shared): ONE launch from now on\n");
        }
    }
    ts->rec_checked = ts->plan.launches;
    if (any) {
        ++m->stat_train_give_ups;           // (statistic "train_give_ups": the caller redoes the step)
        ts->rec_penalty = ts->rec_penalty ? std::min(2 * ts->rec_penalty, 1 << 20) : 16;
        ts->rec_skip = ts->rec_penalty + 1;
        fprintf(stderr, "cor_asv_ann_hip: a persistent recurrence of the train step gave up waiting (is the GPU shared?); "
                        "per-step launches for the next %d steps\n", ts->rec_penalty);
    }
    return 0;
}

// The cell's backward recurrence as ONE launch (train_persist_topb.hip; two side by side in the split form) where the step may
// take a persistent launch and the shape has one; *done says whether it did.  dc: dL/dc, cleared; dL/dc0 at the end.
static int cell_backward_persistent(Step& s, float* dc, bool* done) {
    casv_model* m = s.m; TrainState* ts = s.ts; hipStream_t st = s.st;
    const int B = s.B, T = s.T, U = s.U, W = s.W, C = s.C;
    const int kr = C + W;
    TLayer& top = s.top();
    return persist_launch(m, persist_site(TRAIN_CELL_BWD, {W, C, B, U, 1}, true, T), 2.0 * B * U * ((double)4 * W * (C + W) + (double)W * W), done,
                          [&](const TrainLaunch& plan, unsigned* counters) {
        TopBwdArgs ra{};
        ra.WrT = top.wrT.as<float>(); ra.WaN = ts->WaN.as<float>(); ra.dG = ts->dG.as<float>();
        ra.Gt = top.Gt.as<float>(); ra.Cs = top.Cs.as<float>(); ra.c0 = s.dec_c0(s.D); ra.dZ = top.Z.as<float>(); ra.dRec = top.dRec.as<float>();
        ra.dhatt = ts->dhatt.as<float>(); ra.DWQ = ts->DWQ.as<float>(); ra.WQ = ts->WQ.as<float>(); ra.Ast = ts->Ast.as<float>();
        ra.WIN = ts->WIN.as<int>(); ra.dc_out = dc; ra.B = B; ra.U = U; ra.W = W; ra.C = C; ra.counters = counters;
        AttnBwdArgs& ab = ra.ab;
        ab.mcell = s.mcell; ab.ld_mcell = W + C; ab.mc_off = W; ab.va = ts->W_(ts->iva);
        ab.u = ts->u.as<float>(); ab.u_line = W; ab.u_time = (long long)B * W;
        ab.enc = s.enc_out; ab.enc_line = C; ab.enc_time = (long long)B * C;
        ab.d_enc = ts->d_enc.as<float>(); ab.du = ts->du.as<float>();
        ab.dva_part = ts->dvaP.as<float>(); ab.dbv_part = ts->dbvP.as<float>(); ab.B = B; ab.T = T; ab.W = W; ab.C = C;
        ra.DS = plan.defer ? ts->DSrows.as<float>() : nullptr; ra.defer = plan.defer;
        ra.split_a = plan.split_a;
        if (ra.split_a && !ts->side) {          // (no second stream to be had: one launch, as before)
            if (hipStreamCreateWithFlags(&ts->side, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); ts->side = nullptr; }
            else if (hipEventCreateWithFlags(&ts->ev_fork, hipEventDisableTiming) != hipSuccess ||
                     hipEventCreateWithFlags(&ts->ev_join, hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipStreamDestroy(ts->side); ts->side = nullptr;
            }
            if (!ts->side) { ts->split_off = true; ra.split_a = 0; }
        }
        if (ra.split_a) {
            HIPCHK(hipEventRecord(ts->ev_fork, st));
            HIPCHK(hipStreamWaitEvent(ts->side, ts->ev_fork, 0));
            launch_train_attention_cell_bwd_rows(ra, plan.grid, ts->side);
            HIPCHK(hipEventRecord(ts->ev_join, ts->side));
            ts->split_launch = plan.slot;
        }
        launch_train_attention_cell_bwd(ra, plan.grid, st);
        if (ra.split_a) HIPCHK(hipStreamWaitEvent(st, ts->ev_join, 0));
        if (plan.defer) {
            AttnDeferArgs da{};
            da.dRec = ra.dRec; da.ld_drec = kr; da.mcell = s.mcell; da.ld_mcell = W + C; da.mc_off = W;
            da.Ast = ra.Ast; da.WIN = ra.WIN; da.DS = ra.DS; da.WQ = ra.WQ; da.va = ab.va; da.u = ab.u;
            da.d_enc = ab.d_enc; da.du = ab.du; da.B = B; da.U = U; da.T = T; da.W = W; da.C = C; da.what = plan.defer;
            launch_attention_deferred(da, st);
        }
        return 0;
    });
}

// ... and as three launches per time step (two with the fused backward step): cell backward + data GEMM, attention backward, query GEMM
static int cell_backward_steps(Step& s, float* dc) {
    casv_model* m = s.m; TrainState* ts = s.ts; hipStream_t st = s.st;
    const int B = s.B, T = s.T, U = s.U, W = s.W, C = s.C;
    const int kr = C + W;
    TLayer& top = s.top();
    const float* c0t = s.dec_c0(s.D);
    HIPCHK(hipMemsetAsync(ts->dhatt.p, 0, s.UB * W * 4, st));     // (split-K outputs of the per-step GEMMs; the persistent kernel stores them)
    for (int t = U - 1; t >= 0; --t) {
        LstmBwdArgs p{};
        p.a = ts->dG.as<float>() + (long long)t * B * W; p.lda = W;
        if (t < U - 1) {
            p.b = top.dRec.as<float>() + (long long)(t + 1) * B * kr + C; p.ldb = kr;
            p.c = ts->dhatt.as<float>() + (long long)(t + 1) * B * W; p.ldc = W;
        }
        p.gates = top.Gt.as<float>() + (long long)t * B * 4 * W;
        p.cell = top.Cs.as<float>() + (long long)t * B * W;
        p.c_prev = t > 0 ? top.Cs.as<float>() + (long long)(t - 1) * B * W : c0t; p.ld_cprev = W;
        p.dc = dc; p.dz = top.Z.as<float>() + (long long)t * B * 4 * W; p.rows = B; p.W = W;
        float* drec = top.dRec.as<float>() + (long long)t * B * kr;
        if (s.fused) {
            BwdStepBatch fb{};
            fb.count = 1;
            BwdStepJob& q = fb.j[0];
            q.p = p;
            q.dc_in = ((U - 1 - t) & 1) ? ts->dcalt.as<float>() : dc; q.p.dc = ((U - 1 - t) & 1) ? dc : ts->dcalt.as<float>();
            q.Bt = top.wrT.as<float>(); q.out = drec; q.ld_out = kr; q.N = kr;
            hipEvent_t ev{};
            m->prof_begin(PC_GEMM, 2.0 * B * (double)kr * 4.0 * W, 4.0 * ((double)B * 4 * W + (double)kr * 4 * W + (double)B * kr), ev);
            launch_lstm_bwd_gemm(fb, st);
            m->prof_end(PC_GEMM, ev);
        } else {
            launch_lstm_bwd(p, st);
            GemmArgs g = plain_gemm(p.dz, 4 * W, B, 4 * W, top.wrT.as<float>(), kr, nullptr, drec, kr); g.out_zeroed = 1; run_gemm(m, EPI_PLAIN, g);
        }
        AttnBwdArgs ab{};
        ab.dxh = drec; ab.ld_dxh = kr; ab.ctx_off = 0; ab.mcell = s.mcell; ab.ld_mcell = W + C; ab.mc_off = W;
        ab.a = ts->Ast.as<float>() + (long long)(t + 1) * B * T; ab.win = ts->WIN.as<int>() + (long long)t * B;
        ab.wq = ts->WQ.as<float>() + (long long)t * B * W; ab.va = ts->W_(ts->iva);
        ab.u = ts->u.as<float>(); ab.u_line = W; ab.u_time = (long long)B * W;
        ab.enc = s.enc_out; ab.enc_line = C; ab.enc_time = (long long)B * C;
        ab.d_enc = ts->d_enc.as<float>(); ab.du = ts->du.as<float>(); ab.dwq = ts->DWQ.as<float>() + (long long)t * B * W;
        ab.dva_part = ts->dvaP.as<float>(); ab.dbv_part = ts->dbvP.as<float>(); ab.B = B; ab.T = T; ab.W = W; ab.C = C;
        launch_attention_bwd(ab, st, s.det);
        GemmArgs g = plain_gemm(ab.dwq, W, B, W, ts->WaN.as<float>(), W, nullptr, ts->dhatt.as<float>() + (long long)t * B * W, W);
        g.out_zeroed = 1;
        run_gemm(m, EPI_PLAIN, g);
    }
    if (s.fused && (U & 1)) HIPCHK(hipMemcpyAsync(dc, ts->dcalt.p, (size_t)B * W * 4, hipMemcpyDeviceToDevice, st));   // dL/dc0 of the cell
    return 0;
}

// Phase 6 leaves the tied projection's gradient, dL/d(cell input sequence) in dXtop, dL/d(attended sequence) in d_enc, the
// gradients of the cell's and the attention's parameters, and dL/dh0, dL/dc0 of the cell in dfin_h(D), dfin_c(D).
static int backward_cell(Step& s) {
    casv_model* m = s.m; TrainState* ts = s.ts; hipStream_t st = s.st;
    const int B = s.B, W = s.W, V = s.V, Vp = s.Vp, C = s.C, D = s.D;
    const long long TB = s.TB, UB = s.UB;
    const int kr = C + W;
    TLayer& top = s.top();
    float* dlog = ts->logits.as<float>();
    // tied projection: dE += dlogits^T . G ; dG = dlogits . E
    {
        run_gemm_tn(m, dlog, Vp, Vp, V, s.proj_in, s.proj_ld, W, UB, ts->G_(ts->iE), W);      // (the padding columns of dlogits are zero)
        GemmArgs g2 = plain_gemm(dlog, Vp, (int)UB, Vp, ts->ETp.as<float>(), W, nullptr, ts->dG.as<float>(), W);
        run_plain(m, g2);
    }
    HIPCHK(hipMemsetAsync(ts->d_enc.p, 0, TB * C * 4, st));
    HIPCHK(hipMemsetAsync(ts->du.p, 0, TB * W * 4, st));
    HIPCHK(hipMemsetAsync(ts->dvaP.p, 0, (size_t)B * W * 4, st));
    for (auto& l : ts->layers) if (!l.drec_cleared) HIPCHK(hipMemsetAsync(l.dRec.p, 0, (size_t)l.len * B * l.kr * 4, st));
    HIPCHK(hipMemsetAsync(ts->dbvP.p, 0, (size_t)B * 4, st));
    float* dc = s.dfin_c(D);
    HIPCHK(hipMemsetAsync(dc, 0, (size_t)B * W * 4, st));
    bool topb_persistent = false;
    if (int rc = cell_backward_persistent(s, dc, &topb_persistent)) return rc;
    if (!topb_persistent) if (int rc = cell_backward_steps(s, dc)) return rc;
    launch_colsum(ts->dvaP.as<float>(), B, W, W, ts->G_(ts->iva), st, s.det);
    launch_colsum(ts->dbvP.as<float>(), B, 1, 1, ts->G_(ts->ibv), st, s.det);
    // dL/dh0 of the cell = recurrent part of step 0 + the query path of step 0
    launch_mul_mask(top.dRec.as<float>() + C, kr, nullptr, s.dfin_h(D), W, B, W, st);
    launch_axpy(s.dfin_h(D), ts->dhatt.as<float>(), (long long)B * W, st);       // slot of step 0
    // y-part gradient for all steps, weight grads
    GemmArgs g = plain_gemm(top.Z.as<float>(), 4 * W, (int)UB, 4 * W, top.wxT.as<float>(), W, nullptr, ts->dXtop.as<float>(), W);
    run_plain(m, g);
    launch_mul_rowmask(ts->dXtop.as<float>(), W, s.mcell, W + C, ts->dXtop.as<float>(), W, UB, B, W, st);
    if (s.res_top()) launch_axpy(ts->dXtop.as<float>(), ts->dG.as<float>(), UB * W, st);       // the sum's other branch: dL/d(cell input sequence) += dL/d(projection input)
    if (int rc = layer_weight_grads(m, top, ts->Ym.as<float>(), W, ts->RecIn.as<float>(), kr)) return rc;
    // attention parameters: dWaT = DWQ^T . Hprev ; dbUW = colsum(DWQ) ; u path
    if (!ts->tens[ts->iWaT].frozen) {
        // the h_prev of every step are columns C.. of the cell's recurrent-side inputs
        run_gemm_tn(m, ts->DWQ.as<float>(), W, W, W, ts->RecIn.as<float>() + C, kr, W, UB, ts->G_(ts->iWaT), W, ts->G_(ts->ibUW));
    }
    {
        run_gemm_tn(m, ts->du.as<float>(), W, W, W, s.enc_out, C, C, TB, ts->G_(ts->iUT), C);
        GemmArgs gd = plain_gemm(ts->du.as<float>(), W, (int)TB, W, ts->UaN.as<float>(), C, nullptr, ts->d_enc.as<float>(), C, 1);
        run_plain(m, gd);
    }
    return 0;
}

// bridge_dense backward of encoder layer n: dfin_h(n) / dfin_c(n) arrive as gradients w.r.t. the BRIDGED states; through tanh' and the
// Dense layer they become the gradients w.r.t. the layer's own final states (in place), and leave the Dense layers' gradients
static void bridge_backward(Step& s, int n) {
    if (!s.bridged) return;
    casv_model* m = s.m; TrainState* ts = s.ts;
    const int B = s.B, W = s.W;
    for (int s_ = 0; s_ < 2; ++s_) {
        const TrainState::Bridge& br = ts->bridge[2 * (n - 1) + s_];
        float* d = s_ ? s.dfin_c(n) : s.dfin_h(n);
        const float* raw = (s_ ? s.cfin : s.hfin) + (size_t)(n - 1) * B * W;
        const float* post = (s_ ? ts->cbr.as<float>() : ts->hbr.as<float>()) + (size_t)(n - 1) * B * W;
        launch_tanh_bwd(d, post, (long long)B * W, s.st);
        if (!ts->tens[br.ikt].frozen) run_gemm_tn(m, d, W, W, W, raw, W, W, B, ts->G_(br.ikt), W, ts->G_(br.ib));
        GemmArgs g = plain_gemm(d, W, B, W, br.kn.as<float>(), W, nullptr, ts->brtmp.as<float>(), W);
        g.ksplit = 0; g.kgroups = 0;
        run_gemm(m, EPI_PLAIN, g);
        (void)hipMemcpyAsync(d, ts->brtmp.p, (size_t)B * W * 4, hipMemcpyDeviceToDevice, s.st);
    }
}

// Phase 7 leaves the gradients of every layer below the cell, of the bridges and of the embedding (decoder inputs, encoder inputs).
static int backward_layers(Step& s) {
    casv_model* m = s.m; TrainState* ts = s.ts; hipStream_t st = s.st;
    const int B = s.B, T = s.T, U = s.U, A = s.A, W = s.W, V = s.V, C = s.C, D = s.D;
    const long long TB = s.TB, UB = s.UB;
    const bool deep = s.deep, residual = s.residual;
    TLayer* Lfw = &ts->layers[0]; TLayer* Lbw = &ts->layers[1];
    bridge_backward(s, D);
    // ---- decoder layer n with encoder layer n+1 (the mirror of the forward pairing) ----
    const float* dy = ts->dXtop.as<float>();        // gradient w.r.t. DO[D-1] (or Y0 when D == 1)
    const float* dO = ts->d_enc.as<float>();        // gradient w.r.t. O[D]
    long long ld_dO = C;
    // (a pair's input gradients are the next pair's output gradients: two buffers per chain taking turns, nothing is copied)
    float* dy_bufs[2] = {ts->dXtop.as<float>(), ts->dYl.as<float>()}; int dy_cur = 0;
    float* do_bufs[2] = {ts->dXl.as<float>(), ts->dOin.as<float>()}; int do_out = 0;
    for (int n = D - 1; n >= 1 && deep; --n) {
        TLayer& ld = s.dec_layer(n);
        TLayer& lf = s.enc_dir(n + 1, 0); TLayer& lb = s.enc_dir(n + 1, 1);
        const float* xin = n == 1 ? ts->Y0.as<float>() : ts->DO[n - 1].as<float>();
        const bool res_d = residual && n >= 2;
        if (res_d) launch_mul_mask(dy, W, s.mdec_n(n), dy_bufs[dy_cur ^ 1], W, UB, W, st);
        {
            LayerBwd one[1] = {{&ld, dy, W, s.mdec_n(n), nullptr, nullptr, s.dec_h0(n), s.dec_c0(n), s.dfin_c(n),
                                xin, W, dy_bufs[dy_cur ^ 1], W, res_d ? 1 : 0}};
            if (int rc = layers_backward(m, one, 1)) return rc;
        }
        HIPCHK(hipMemcpyAsync(s.dfin_h(n), ld.dRec.as<float>(), (size_t)B * W * 4, hipMemcpyDeviceToDevice, st));
        bridge_backward(s, n);
        dy_cur ^= 1; dy = dy_bufs[dy_cur];
        // the BiLSTM n + 1: forward direction takes columns [0,W) of dO, backward direction [W,2W); both add into the gradient of their
        // shared input, whose cross sum (the Lambda is its own adjoint) is the gradient w.r.t. O[n]
        float* dXn = do_bufs[0]; float* dOn = do_bufs[1];
        LayerBwd pair[2] = {
            {&lf, dO, ld_dO, s.menc_n(n + 1), nullptr, nullptr, nullptr, nullptr, ts->dcbuf.as<float>(),
             ts->XD[n + 1].as<float>(), 2 * W, dXn, 2 * W, 0},
            {&lb, dO + W, ld_dO, s.menc_n(n + 1) ? s.menc_n(n + 1) + W : nullptr, s.dfin_h(n + 1), s.dfin_c(n + 1), nullptr, nullptr, ts->dcbuf2.as<float>(),
             ts->XD[n + 1].as<float>(), 2 * W, dXn, 2 * W, 1}};
        if (int rc = layers_backward(m, pair, 2)) return rc;
        launch_cross_sum(dXn, dOn, TB * 2 * W, st);
        dO = dOn; ld_dO = 2 * W;
    }
    for (int n = D - 1; n >= 1 && !deep; --n) {
        TLayer& ld = s.dec_layer(n);
        TLayer& le = s.enc_layer(n + 1);
        const float* xin = n == 1 ? ts->Y0.as<float>() : ts->DO[n - 1].as<float>();
        // residual_connections: decoder layer n >= 2 / encoder layer n + 1 >= 3 pass their output gradient (times the mask) straight on to
        // their input as well: the input-gradient buffers start from it and the layers' data gradients are added
        const bool res_d = residual && n >= 2, res_e = residual && n + 1 >= 3;
        if (res_d) launch_mul_mask(dy, W, s.mdec_n(n), dy_bufs[dy_cur ^ 1], W, UB, W, st);
        if (res_e) launch_mul_mask(dO, ld_dO, s.menc_n(n + 1), do_bufs[do_out], le.kx, TB, W, st);
        LayerBwd pair[2] = {
            {&ld, dy, W, s.mdec_n(n), nullptr, nullptr, s.dec_h0(n), s.dec_c0(n), s.dfin_c(n),
             xin, W, dy_bufs[dy_cur ^ 1], W, res_d ? 1 : 0},
            {&le, dO, ld_dO, s.menc_n(n + 1), s.dfin_h(n + 1), s.dfin_c(n + 1), nullptr, nullptr, ts->dcbuf.as<float>(),
             ts->O[n].as<float>(), le.kx, do_bufs[do_out], le.kx, res_e ? 1 : 0}};
        if (int rc = layers_backward(m, pair, 2)) return rc;
        // dL/dh0, dL/dc0 of the decoder layer go to the encoder layer of the same index
        HIPCHK(hipMemcpyAsync(s.dfin_h(n), ld.dRec.as<float>(), (size_t)B * W * 4, hipMemcpyDeviceToDevice, st));
        bridge_backward(s, n);
        dy_cur ^= 1; dy = dy_bufs[dy_cur];
        dO = do_bufs[do_out]; ld_dO = le.kx; do_out ^= 1;
    }
    if (s.det) launch_embed_segments(ts->G_(ts->iE), ts->seg_dec_off.as<int>(), ts->seg_dec_pos.as<int>(), nullptr, dy, W, B, U, 1, V, W, st);
    else launch_embed_scatter(ts->G_(ts->iE), ts->d_in.as<int>(), nullptr, dy, W, B, U, 1, V, W, st);

    // ---- encoder layer 1: forward direction takes columns [0,W) of dO1, backward direction [W,2W) ----
    {
        LayerBwd pair[2] = {
            {Lfw, dO, ld_dO, s.menc_n(1), nullptr, nullptr, nullptr, nullptr, ts->dcbuf.as<float>(),
             ts->X0.as<float>(), W, ts->dX0.as<float>(), W, 0},
            {Lbw, dO + W, ld_dO, s.menc_n(1) ? s.menc_n(1) + W : nullptr, s.dfin_h(1), s.dfin_c(1), nullptr, nullptr, ts->dcbuf2.as<float>(),
             ts->X0.as<float>(), W, ts->dX0.as<float>(), W, 1}};
        if (int rc = layers_backward(m, pair, 2)) return rc;
    }
    if (s.det) launch_embed_segments(ts->G_(ts->iE), ts->seg_enc_off.as<int>(), ts->seg_enc_pos.as<int>(), s.enc_val ? ts->e_val.as<float>() : nullptr,
                                     ts->dX0.as<float>(), W, B, T, A, V, W, st);
    else launch_embed_scatter(ts->G_(ts->iE), ts->e_idx.as<int>(), s.enc_val ? ts->e_val.as<float>() : nullptr, ts->dX0.as<float>(), W, B, T, A, V, W, st);
    return 0;
}

// One launch over all parameter tensors that are not frozen; lists of MULTI_MAX tensors at a time
template <class Launch> static void over_tensors(TrainState* ts, int max_blocks, Launch&& launch) {
    MultiTensor mt{};
    for (auto& t : ts->tens) {
        if (t.frozen) continue;
        if (mt.count == MULTI_MAX) { launch(mt); mt = MultiTensor{}; }
        multi_add(mt, t.w.as<float>(), t.g.as<float>(), t.m.as<float>(), t.v.as<float>(), (long long)t.n, max_blocks);
    }
    launch(mt);
}

// Phase 8 leaves the regulariser in the loss and the embedding's gradient, the gradients' norm, (mode 1) the clipped Adam update with
// the derived layouts refreshed, and the step's loss and norm with the caller.
static int update(Step& s, double* loss_out, double* norm_out) {
    casv_model* m = s.m; TrainState* ts = s.ts; hipStream_t st = s.st;
    double* parts = s.parts;
    launch_reg(ts->W_(ts->iE), ts->G_(ts->iE), s.V, s.W, ts->loss.as<double>(), 1, st, parts);
    // (few workgroups per tensor: every one of them ends in an atomic add on the ONE sum -- ~12 ns each, one after the other)
    over_tensors(ts, 64, [&](const MultiTensor& mt) { launch_sumsq_multi(mt, ts->normsq.as<double>(), st, parts); });
    if (s.mode == 1) {
        ts->step += 1;
        const double b1 = ts->ap.beta1, b2 = ts->ap.beta2;
        const float lr_t = (float)(ts->ap.lr * sqrt(1.0 - pow(b2, (double)ts->step)) / (1.0 - pow(b1, (double)ts->step)));
        over_tensors(ts, 2048, [&](const MultiTensor& mt) {
            launch_adam_multi(mt, ts->normsq.as<double>(), ts->ap.clipnorm, lr_t, (float)b1, (float)b2, ts->ap.epsilon, st);
        });
        refresh_derived(m, ts);
    }
    double nsq = 0.0;
    HIPCHK(hipMemcpyAsync(loss_out, ts->loss.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&nsq, ts->normsq.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    if (norm_out) *norm_out = sqrt(nsq);
    if (m->prof.on) m->prof.collect();
    return CASV_OK;
}

// One attempt at the step, the phases in order.  *redo: a persistent recurrence gave up -- nothing has been updated, the back-off is
// set (recurrences_gave_up) and the caller starts over.
int train_attempt(Step s, double* loss_out, double* norm_out, bool* redo) {
    casv_model* m = s.m; TrainState* ts = s.ts;
    ts->B = s.B; ts->Be = s.Be; ts->N = s.N; ts->T = s.T; ts->U = s.U; ts->A = s.A;
    ts->score_B = 0;                       // (a scoring call's attention rows are overwritten)
    m->encoded = false;                    // the final-state buffers are shared with the inference session
    if (int rc = plan_buffers(s)) return rc;
    if (int rc = stage_inputs(s)) return rc;
    if (int rc = forward_layers(s)) return rc;
    if (int rc = forward_cell(s)) return rc;
    if (int rc = s.sched ? sched_passes(s) : 0) return rc;          // (casv_train_step_sampled: train_sched.hip)
    if (int rc = loss_head(s)) return rc;
    if (int rc = recurrences_gave_up(m, *redo)) return rc;
    if (*redo) return CASV_OK;
    if (!s.training) {                     // K.in_train_phase: the regulariser counts only in the train phase
        HIPCHK(hipMemcpyAsync(loss_out, ts->loss.p, 8, hipMemcpyDeviceToHost, s.st));
        HIPCHK(hipStreamSynchronize(s.st));
        if (norm_out) *norm_out = 0.0;
        m->stat_train_launches = ts->plan.launches;
        return CASV_OK;
    }
    if (int rc = backward_cell(s)) return rc;
    if (int rc = backward_layers(s)) return rc;
    if (int rc = recurrences_gave_up(m, *redo)) return rc;
    if (*redo) return CASV_OK;
    if (ts->plan.launches) ts->rec_penalty = 0;
    if (ts->tn_ws_rc) {                    // (a weight gradient was not computed: no update, the step fails with the allocation's error)
        (void)hipStreamSynchronize(s.st);
        return ts->tn_ws_rc;
    }
    if (int rc = update(s, loss_out, norm_out)) return rc;
    m->stat_train_launches = ts->plan.launches;      // (statistic "train_persistent_launches"; a step redone per step ends here with 0)
    return CASV_OK;
}

// The view of a step of Be lines with N decoder rows each (the targets are the entry's to add): what the caller passed, the model's
// shapes, the step's flags.
Step step_view(casv_model* m, const StepArgs& a, int Be, int N) {
    Step s{};
    s.m = m; s.ts = m->train; s.st = m->stream;
    s.mode = a.mode; s.B = Be * N; s.Be = Be; s.N = N; s.T = a.T; s.U = a.U; s.A = a.A;
    s.enc_idx = a.enc_idx; s.enc_val = a.enc_val; s.dec_in = a.dec_in; s.weights = a.weights;
    s.mask_enc = a.mask_enc; s.mask_dec = a.mask_dec; s.mask_cell = a.mask_cell;
    s.W = m->W; s.V = m->V; s.Vp = m->Vp; s.C = m->C; s.D = m->D;
    s.TB = (long long)a.T * Be; s.UB = (long long)a.U * s.B;
    s.training = a.mode != 0; s.det = m->deterministic; s.fused = m->fused_backward && !s.det;
    s.deep = m->cfg.deep_bidirectional_encoder != 0 && s.D >= 2;
    s.residual = m->cfg.residual_connections != 0; s.bridged = m->cfg.bridge_dense != 0;
    return s;
}

// What every step entry refuses, in this order (own_pointers: the entry's own arguments are there; modes min_mode .. 2 pass).
int check_step_args(const casv_model* m, const StepArgs& a, bool own_pointers, int min_mode, const char* mode_message) {
    if (!m || !a.enc_idx || !a.dec_in || !own_pointers || !a.weights || !a.loss_out) return fail(CASV_ERR_ARG, "null argument");
    if (!m->train) return fail(CASV_ERR_STATE, "casv_train_begin must run first");
    if (a.B < 1 || a.T < 1 || a.U < 1 || a.A < 1) return fail(CASV_ERR_ARG, "bad shape");
    if (a.mode < min_mode || a.mode > 2) return fail(CASV_ERR_ARG, "%s", mode_message);
    return CASV_OK;
}

// The body of every step entry behind its checks: the scopes that make the step's bits a function of the options alone, its view
// with the entry's fields (fill), at most two attempts, what the entry takes from a finished one (done).
int run_step(casv_model* m, const StepArgs& a, const StepHook& fill, const StepHook& done) {
    HIPCHK(hipSetDevice(m->device));
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_TRAIN));       // (engine.h: the whole-sequence contractions with a split form take the bf16x3-split arithmetic)
    OrderedScope ordered(m, m->deterministic);
    Step s = step_view(m, a, a.B, 1);
    if (int rc = fill(s)) return rc;
    // A persistent recurrence that gave up (in a scheduled-sampling pass too) sets the back-off: the second attempt takes per-step launches only.
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool redo = false;
        if (int rc = train_attempt(s, a.loss_out, a.norm_out, &redo)) return rc;
        if (!redo) return done ? done(s) : CASV_OK;
    }
    return fail(CASV_ERR_STATE, "the train step gave up twice: its second attempt took a persistent launch");
}
}  // namespace casv

static const char* const kStepModes = "mode must be 0 (evaluate), 1 (train) or 2 (gradients only)";

extern "C" int casv_train_step(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                               const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                               const float* weights, const float* mask_enc, const float* mask_dec, const float* mask_cell,
                               double* loss_out, double* norm_out) {
    const StepArgs a{mode, B, T, U, A, enc_idx, enc_val, dec_in, weights, mask_enc, mask_dec, mask_cell, loss_out, norm_out};
    if (int rc = check_step_args(m, a, dec_out, 0, kStepModes)) return rc;
    // (run_step's body spelled out: tests/test_train_form_cases.py reads the step's launch order from this function's text)
    HIPCHK(hipSetDevice(m->device));
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_TRAIN));
    OrderedScope ordered(m, m->deterministic);
    Step s = step_view(m, a, B, 1); s.dec_out = dec_out;
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool redo = false;
        if (int rc = train_attempt(s, loss_out, norm_out, &redo)) return rc;
        if (!redo) return CASV_OK;
    }
    return fail(CASV_ERR_STATE, "the train step gave up twice: its second attempt took a persistent launch");
}

// The soft targets' rules (include/cor_asv_ann_hip.h), checked on the host before anything is launched or cleared: O(B*U*K).
int check_soft_targets(long long positions, int K, int V, const int32_t* soft_idx, const float* soft_q) {
    if (K < 1 || K > V || K > 64) return fail(CASV_ERR_ARG, "K=%d outside [1, min(V, 64)] = [1, %d]", K, V < 64 ? V : 64);
    for (long long p = 0; p < positions; ++p) {
        const int32_t* ix = soft_idx + p * K; const float* q = soft_q + p * K;
        for (int k = 0; k < K; ++k) {
            if (ix[k] < -1 || ix[k] >= V) return fail(CASV_ERR_ARG, "soft_idx[%lld][%d] = %d outside [-1, %d)", p, k, ix[k], V);
            if (ix[k] < 0) continue;
            if (!(q[k] >= 0.f) || q[k] == INFINITY) return fail(CASV_ERR_ARG, "soft_q[%lld][%d] = %g: a mass is finite and >= 0", p, k, (double)q[k]);
            for (int j = 0; j < k; ++j)
                if (ix[j] == ix[k]) return fail(CASV_ERR_ARG, "soft_idx[%lld]: index %d in slots %d and %d", p, ix[k], j, k);
        }
    }
    return CASV_OK;
}

// casv_train_step with the target array replaced by K (index, mass) slots per position.
extern "C" int casv_train_step_soft(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                                    const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, int32_t K,
                                    const int32_t* soft_idx, const float* soft_q, const float* weights, const float* mask_enc,
                                    const float* mask_dec, const float* mask_cell, double* loss_out, double* norm_out) {
    const StepArgs a{mode, B, T, U, A, enc_idx, enc_val, dec_in, weights, mask_enc, mask_dec, mask_cell, loss_out, norm_out};
    if (int rc = check_step_args(m, a, soft_idx && soft_q, 0, kStepModes)) return rc;
    if (int rc = check_soft_targets((long long)B * U, K, m->V, soft_idx, soft_q)) return rc;
    return run_step(m, a, [&](Step& s) { s.K = K; s.soft_idx = soft_idx; s.soft_q = soft_q; return 0; });
}

// The risk head's rules (include/cor_asv_ann_hip.h), checked on the host before anything is launched or cleared: O(B).  *inv = 1 /
// max(number of groups with at least one member, 1).
int check_risk(int B, int N, const float* cost, double alpha, double* inv) {
    if (N < 1 || N > 64 || B % N) return fail(CASV_ERR_ARG, "N=%d: 1 <= N <= 64 and B=%d a multiple of N", N, B);
    if (!cost) return fail(CASV_ERR_ARG, "null argument");
    if (!(alpha > 0.0) || alpha == (double)INFINITY) return fail(CASV_ERR_ARG, "alpha = %g: finite and > 0", alpha);
    long groups = 0;
    for (int g = 0; g < B / N; ++g) {
        bool any = false;
        for (int i = 0; i < N; ++i) {
            const float c = cost[(size_t)g * N + i];
            if (c != c || c == INFINITY || c == -INFINITY) return fail(CASV_ERR_ARG, "cost[%d] = %g: a cost is finite (negative: not a member)", g * N + i, (double)c);
            any |= c >= 0.f;
        }
        groups += any;
    }
    *inv = 1.0 / (double)std::max(groups, 1L);
    return CASV_OK;
}

// casv_train_step with the minimum-risk head in place of the cross-entropy; a finished step hands over the head's q and risks.
extern "C" int casv_train_step_risk(casv_model* m, int32_t mode, int32_t B, int32_t T, int32_t U, int32_t A,
                                    const int32_t* enc_idx, const float* enc_val, const int32_t* dec_in, const int32_t* dec_out,
                                    const float* weights, const float* mask_enc, const float* mask_dec, const float* mask_cell,
                                    int32_t N, const float* cost, double alpha, double* out_q, double* out_risk,
                                    double* loss_out, double* norm_out) {
    const StepArgs a{mode, B, T, U, A, enc_idx, enc_val, dec_in, weights, mask_enc, mask_dec, mask_cell, loss_out, norm_out};
    if (int rc = check_step_args(m, a, dec_out, 1, "mode must be 1 (train) or 2 (gradients only): the risk has no evaluation form")) return rc;
    double inv = 1.0;
    if (int rc = check_risk(B, N, cost, alpha, &inv)) return rc;
    return run_step(m, a, [&](Step& s) { s.dec_out = dec_out; s.RN = N; s.cost = cost; s.alpha = alpha; s.inv_groups = inv; return 0; },
        [&](Step& s) {                         // (the attempt has waited for the stream)
            if (out_q) HIPCHK(hipMemcpy(out_q, s.ts->r_q.p, (size_t)B * 8, hipMemcpyDeviceToHost));
            if (out_risk) HIPCHK(hipMemcpy(out_risk, s.ts->r_risk.p, (size_t)(B / N) * 8, hipMemcpyDeviceToHost));
            return 0;
        });
}

// Test support: one backward time step of 1 or 2 layers on host data (casv_debug_bwd_step), in the fused form or as the two
// launches layers_backward and cell_backward_steps build.  Nothing is launched unless every address the kernels form lies inside
// a buffer allocated here: they clamp rows to rows - 1 and columns to N - 1, read W floats of every input row ([rows][ld], the
// last row W floats long) and of the mask, 4W of a gates row and of a Bt row; they store rows < rows only.
namespace {
int check_debug_bwd_job(const casv_debug_bwd_job& d, int j, int W0) {
    if (d.rows < 1 || d.rows > (1 << 16) || d.N < 1 || d.N > (1 << 14)) return fail(CASV_ERR_ARG, "job %d: rows in [1, 65536], N in [1, 16384]", j);
    if (d.W < 32 || d.W > 1024 || d.W % 32 || d.W != W0) return fail(CASV_ERR_ARG, "job %d: W a multiple of 32 in [32, 1024], the same in every job", j);
    if (!d.Bt || !d.gates || !d.cell || !d.dc_in || !d.dz || !d.dc || !d.out) return fail(CASV_ERR_ARG, "job %d: Bt, gates, cell, dc_in, dz, dc and out are required", j);
    if (d.mask_a && !d.a) return fail(CASV_ERR_ARG, "job %d: mask_a without a", j);
    const struct { const float* p; int64_t ld; int width; const char* name; } lds[5] = {
        {d.a, d.lda, d.W, "lda"}, {d.b, d.ldb, d.W, "ldb"}, {d.c, d.ldc, d.W, "ldc"}, {d.c_prev, d.ld_cprev, d.W, "ld_cprev"}, {d.out, d.ld_out, d.N, "ld_out"}};
    for (const auto& l : lds)
        if (l.p && (l.ld < l.width || l.ld % 4 || l.ld > (1 << 16))) return fail(CASV_ERR_ARG, "job %d: %s must be >= %d, a multiple of 4 and <= 65536", j, l.name, l.width);
    return CASV_OK;
}
}  // namespace

extern "C" int casv_debug_bwd_step(casv_model* m, int32_t form, int32_t count, const casv_debug_bwd_job* jobs) {
    if (!m || !jobs) return fail(CASV_ERR_ARG, "null argument");
    if ((form != 0 && form != 1) || count < 1 || count > 2) return fail(CASV_ERR_ARG, "form 0 (fused) / 1 (two launches), 1 or 2 jobs");
    for (int j = 0; j < count; ++j) if (int rc = check_debug_bwd_job(jobs[j], j, jobs[0].W)) return rc;
    HIPCHK(hipSetDevice(m->device));
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_TRAIN));
    OrderedScope ordered(m, m->deterministic);          // (as casv_train_step: form 1's GEMM then sums in a fixed order)
    DebugBuffers dev{m->stream};
    int rc = CASV_OK;
    auto put = [&](const float* src, size_t n) { return static_cast<float*>(dev.put(src, n, rc)); };     // n floats: a copy of src, or (nullptr) 0xFF bytes
    BwdStepBatch fb{};
    LstmBwdBatch pw{};
    GemmBatch gb{};
    fb.count = pw.count = gb.count = count;
    for (int j = 0; j < count; ++j) {
        const casv_debug_bwd_job& d = jobs[j];
        const size_t rows = (size_t)d.rows, W = (size_t)d.W;
        auto in = [&](const float* src, int64_t ld) -> const float* { return src ? put(src, (rows - 1) * (size_t)ld + W) : nullptr; };
        BwdStepJob& q = fb.j[j];
        LstmBwdArgs& p = q.p;
        p.a = in(d.a, d.lda); if (rc) return rc;
        p.lda = d.lda;
        if (d.mask_a) { p.mask_a = put(d.mask_a, W); if (rc) return rc; }
        p.b = in(d.b, d.ldb); if (rc) return rc;
        p.ldb = d.ldb;
        p.c = in(d.c, d.ldc); if (rc) return rc;
        p.ldc = d.ldc;
        p.c_prev = in(d.c_prev, d.ld_cprev); if (rc) return rc;
        p.ld_cprev = d.ld_cprev;
        p.gates = put(d.gates, rows * 4 * W); if (rc) return rc;
        p.cell = put(d.cell, rows * W); if (rc) return rc;
        q.dc_in = put(d.dc_in, rows * W); if (rc) return rc;
        q.Bt = put(d.Bt, (size_t)d.N * 4 * W); if (rc) return rc;
        // outputs: 0xFF bytes and one guard row; out[:rows][:N] cleared (the split-K shares add into it)
        p.dz = put(nullptr, (rows + 1) * 4 * W); if (rc) return rc;
        p.dc = put(nullptr, (rows + 1) * W); if (rc) return rc;
        q.out = put(nullptr, (rows + 1) * (size_t)d.ld_out); if (rc) return rc;
        q.ld_out = d.ld_out; q.N = d.N; p.rows = d.rows; p.W = d.W;
        HIPCHK(hipMemset2DAsync(q.out, (size_t)d.ld_out * 4, 0, (size_t)d.N * 4, rows, m->stream));
        if (form == 1) {            // lstm_bwd_kernel works in place: dL/dc of the step lies where dL/dc of the step before goes
            HIPCHK(hipMemcpyAsync(p.dc, q.dc_in, rows * W * 4, hipMemcpyDeviceToDevice, m->stream));
            pw.a[j] = p;
            gb.g[j] = plain_gemm(p.dz, 4 * d.W, d.rows, 4 * d.W, q.Bt, d.N, nullptr, q.out, d.ld_out);
            gb.g[j].out_zeroed = 1;
        }
    }
    m->stat_bwd_step[0] = m->stat_bwd_step[1] = 0;
    if (form == 0) {
        const BwdStepPlan plan = launch_lstm_bwd_gemm(fb, m->stream);
        m->stat_bwd_step[0] = plan.ksplit; m->stat_bwd_step[1] = plan.gper;
    } else {
        launch_lstm_bwd_batch(pw, m->stream);
        run_gemm_batch(m, EPI_PLAIN, gb);
    }
    HIPCHK(hipGetLastError());
    for (int j = 0; j < count; ++j) {
        const casv_debug_bwd_job& d = jobs[j];
        const size_t rows1 = (size_t)d.rows + 1, W = (size_t)d.W;
        HIPCHK(hipMemcpyAsync(d.dz, fb.j[j].p.dz, rows1 * 4 * W * 4, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(d.dc, fb.j[j].p.dc, rows1 * W * 4, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(d.out, fb.j[j].out, rows1 * (size_t)d.ld_out * 4, hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    for (int j = 0; j < count; ++j) {
        const casv_debug_bwd_job& d = jobs[j];
        const size_t rows = (size_t)d.rows, W = (size_t)d.W, ld = (size_t)d.ld_out;
        auto untouched = [](const float* p, size_t n) {
            for (size_t i = 0; i < n; ++i) { uint32_t v; memcpy(&v, p + i, 4); if (v != 0xffffffffu) return false; }
            return true;
        };
        if (!untouched(d.dz + rows * 4 * W, 4 * W)) return fail(CASV_ERR_STATE, "job %d: a launch stored past the last row of dz", j);
        if (!untouched(d.dc + rows * W, W)) return fail(CASV_ERR_STATE, "job %d: a launch stored past the last row of dc", j);
        if (!untouched(d.out + rows * ld, ld)) return fail(CASV_ERR_STATE, "job %d: a launch stored past the last row of out", j);
        for (size_t r = 0; r < rows; ++r)
            if (!untouched(d.out + r * ld + d.N, ld - d.N)) return fail(CASV_ERR_STATE, "job %d: a launch stored behind column N - 1 of out, row %zu", j, r);
    }
    return CASV_OK;
}
