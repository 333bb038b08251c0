// Host side of the C ABI (include/cor_asv_ann_hip.h): the handle, weight repacking, result records, statistics, profile, debug entry
// points and options.  The decode entry points are decode.hip, the encoder pass (seq2seq.py:237-314) encoder.hip, the training session train_state.hip, its step train.hip, scoring score.hip, the row heads' test entries debug_rows.hip.
#include "engine.h"

static std::map<std::string, size_t> expected_shapes(const casv_config& c) {
    const size_t W = c.width, V = c.voc_size, D = c.depth, C = ((D == 1 || c.deep_bidirectional_encoder) ? 2 * W : W);
    std::map<std::string, size_t> m;
    m["E"] = V * W;
    for (const char* d : {"fw", "bw"}) {
        m[std::string("enc1_") + d + "_K"] = W * 4 * W; m[std::string("enc1_") + d + "_R"] = W * 4 * W;
        m[std::string("enc1_") + d + "_b"] = 4 * W;
    }
    for (size_t n = 2; n <= D; ++n) {
        const size_t nin = n == 2 ? 2 * W : W; const std::string p = "enc" + std::to_string(n);
        if (c.deep_bidirectional_encoder) {          // every layer bidirectional, 2W-wide inputs (seq2seq.py:273-276)
            for (const char* d : {"_fw", "_bw"}) { m[p + d + "_K"] = 2 * W * 4 * W; m[p + d + "_R"] = W * 4 * W; m[p + d + "_b"] = 4 * W; }
            continue;
        }
        m[p + "_K"] = nin * 4 * W; m[p + "_R"] = W * 4 * W; m[p + "_b"] = 4 * W;
    }
    m["att_U"] = C * W;
    for (size_t n = 1; n < D; ++n) {
        const std::string p = "dec" + std::to_string(n);
        m[p + "_K"] = W * 4 * W; m[p + "_R"] = W * 4 * W; m[p + "_b"] = 4 * W;
    }
    m["att_Wa"] = W * W; m["att_va"] = W; m["att_bUW"] = W; m["att_bv"] = 1;
    const std::string p = "dec" + std::to_string(D);
    m[p + "_K"] = (W + C) * 4 * W; m[p + "_R"] = W * 4 * W; m[p + "_b"] = 4 * W;
    if (c.bridge_dense)          // Dense(width, tanh) on the final h / c of every encoder layer (seq2seq.py:299-301)
        for (size_t n = 1; n <= D; ++n)
            for (const char* s : {"h", "c"}) {
                const std::string b = "bridge" + std::to_string(n) + "_" + s;
                m[b + "_K"] = W * W; m[b + "_b"] = W;
            }
    return m;
}

extern "C" const char* casv_last_error(void) { return g_err; }
extern "C" const char* casv_version(void) { return "cor_asv_ann_amd 0.1 (gfx950)"; }
extern "C" int casv_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

extern "C" int casv_model_create(const casv_config* cfg, int device_id, casv_model** out) {
    if (!cfg || !out) return fail(CASV_ERR_ARG, "null argument");
    if (cfg->lm || cfg->stateful)
        return fail(CASV_ERR_ARG, "lm_loss/lm_predict and stateful are not implemented (must be off)");
    if (cfg->depth < 1 || cfg->depth > 8) return fail(CASV_ERR_ARG, "depth %d out of range 1..8", cfg->depth);
    if (cfg->width < 32 || cfg->width % 32) return fail(CASV_ERR_ARG, "width %d must be a positive multiple of 32", cfg->width);
    if (cfg->voc_size < 2 || cfg->voc_size > 4096) return fail(CASV_ERR_ARG, "voc_size %d out of range 2..4096", cfg->voc_size);
    if (cfg->window_width < 1 || cfg->window_width > 5) return fail(CASV_ERR_ARG, "window_width %d out of range 1..5", cfg->window_width);
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(CASV_ERR_ARG, "device %d not available (%d devices)", device_id, ndev);
    HIPCHK(hipSetDevice(device_id));
    casv_model* m = new casv_model();
    m->cfg = *cfg; m->device = device_id;
    { hipDeviceProp_t prop{}; if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) m->ncu = prop.multiProcessorCount; }
    m->gemm.ncu = m->ncu;
    // (A/B measurements of a whole program: the defaults of the options "encoder_table" and "beam_skip_last" from the environment)
    if (const char* e = getenv("CASV_ENCODER_TABLE")) m->enc_table_opt = e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1;
    if (const char* e = getenv("CASV_BEAM_SKIP_LAST")) m->beam_skip_last = e[0] != '0';
    m->W = cfg->width; m->V = cfg->voc_size; m->Vp = (cfg->voc_size + 31) & ~31; m->D = cfg->depth;
    m->C = (cfg->depth == 1 || cfg->deep_bidirectional_encoder) ? 2 * cfg->width : cfg->width;
    m->expect = expected_shapes(*cfg);
    hipError_t e = hipStreamCreate(&m->stream);
    if (e != hipSuccess) { delete m; return fail(CASV_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    e = hipEventCreateWithFlags(&m->ev_inputs, hipEventDisableTiming);
    if (e != hipSuccess) { (void)hipStreamDestroy(m->stream); delete m; return fail(CASV_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e)); }
    m->enc.resize(m->D + 1); m->dec.resize(m->D + 1); m->st_h.resize(m->D + 1); m->st_c.resize(m->D + 1);
    m->br_hT.resize(m->D + 1); m->br_hb.resize(m->D + 1); m->br_cT.resize(m->D + 1); m->br_cb.resize(m->D + 1);
    m->enc_dfw.resize(m->D + 1); m->enc_dbw.resize(m->D + 1);
    *out = m;
    return CASV_OK;
}

extern "C" void casv_model_destroy(casv_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->stream);
    for (auto& l : m->dec) gemm_split_invalidate(l.wt.as<float>());
    gemm_split_invalidate(m->WaT.as<float>()); gemm_split_invalidate(m->E.as<float>());
    if (m->pin_in) (void)hipHostFree(m->pin_in);
    if (m->pin_out) (void)hipHostFree(m->pin_out);
    (void)casv_train_release(m);
    (void)casv_score_release(m);
    vendor_gemm_release(m->stream);
    (void)casv_comm_destroy(m);
    if (m->pin_active) { (void)hipHostFree(m->pin_active); for (int k = 0; k < 2; ++k) (void)hipEventDestroy(m->ev_active[k]); }
    if (m->step_exec) (void)hipGraphExecDestroy(m->step_exec);
    if (m->step_graph) (void)hipGraphDestroy(m->step_graph);
    for (auto e : m->prof.pool) (void)hipEventDestroy(e);
    (void)hipEventDestroy(m->ev_inputs);
    (void)hipStreamDestroy(m->stream);
    delete m;              // (every DevBuf of the handle frees itself)
}

extern "C" int casv_set_weight(casv_model* m, const char* name, const float* data, int64_t count) {
    if (!m || !name || !data) return fail(CASV_ERR_ARG, "null argument");
    auto it = m->expect.find(name);
    if (it == m->expect.end()) return fail(CASV_ERR_ARG, "unknown weight '%s' for depth %d", name, m->D);
    if ((size_t)count != it->second) return fail(CASV_ERR_ARG, "weight '%s': expected %zu elements, got %lld", name, it->second, (long long)count);
    m->host[name].assign(data, data + count);
    m->committed = false;
    return CASV_OK;
}

extern "C" int casv_get_weight(casv_model* m, const char* name, float* out, int64_t capacity) {
    if (!m || !name || !out) return fail(CASV_ERR_ARG, "null argument");
    auto it = m->host.find(name);
    if (it == m->host.end()) return fail(CASV_ERR_STATE, "weight '%s' has not been set", name);
    if ((size_t)capacity < it->second.size()) return fail(CASV_ERR_ARG, "buffer too small for '%s'", name);
    memcpy(out, it->second.data(), it->second.size() * sizeof(float));
    return CASV_OK;
}

// K order inside every 16-k tile for the persistent decoder's v_mfma_f32_16x16x4_f32: position 4*kg + q holds the k that
// k group kg contracts in instruction q -- the groups visit k in the order of the 32x32x2 chain of gemm.hip (persist.hip).
static const int kPersistK[4][4] = {{0, 4, 1, 5}, {2, 6, 3, 7}, {8, 12, 9, 13}, {10, 14, 11, 15}};
static void persist_permute_row(const float* src, float* dst, int K) {
    for (int kt = 0; kt < K / 16; ++kt)
        for (int kg = 0; kg < 4; ++kg)
            for (int q = 0; q < 4; ++q) dst[kt * 16 + 4 * kg + q] = src[kt * 16 + kPersistK[q][kg]];
}
// [4W][Kt] gate-interleaved rows ((u/32)*128 + g*32 + u%32) -> [W/16][4][16][Kt] with permuted K; bias likewise
static int pack_persist(casv_model* m, LstmW& dst, const std::vector<float>& wt, const std::vector<float>& bias, int Kt) {
    const int W = m->W;
    std::vector<float> pw((size_t)4 * W * Kt), pb(4 * W);
    for (int u = 0; u < W; ++u)
        for (int g = 0; g < 4; ++g) {
            const int n = (u / 32) * 128 + g * 32 + (u % 32), rowp = ((u / 16) * 4 + g) * 16 + (u % 16);
            persist_permute_row(&wt[(size_t)n * Kt], &pw[(size_t)rowp * Kt], Kt);
            pb[rowp] = bias[n];
        }
    if (int rc = upload(dst.pw, pw)) return rc;
    return upload(dst.pbias, pb);
}

// Keras (in,4W) kernel + (W,4W) recurrent kernel + (4W) bias -> [4W][in+W] rows in the
// gate-interleaved order n = (u/32)*128 + g*32 + u%32, K contiguous.
static int pack_lstm(casv_model* m, LstmW& dst, const std::string& prefix, int kin, bool decoder = false) {
    const int W = m->W, Kt = kin + W;
    const auto& K = m->host[prefix + "_K"]; const auto& R = m->host[prefix + "_R"]; const auto& b = m->host[prefix + "_b"];
    std::vector<float> wt((size_t)4 * W * Kt), bias(4 * W);
    for (int u = 0; u < W; ++u)
        for (int g = 0; g < 4; ++g) {
            const int n = (u / 32) * 128 + g * 32 + (u % 32), col = g * W + u;
            float* row = &wt[(size_t)n * Kt];
            for (int k = 0; k < kin; ++k) row[k] = K[(size_t)k * 4 * W + col];
            for (int k = 0; k < W; ++k) row[kin + k] = R[(size_t)k * 4 * W + col];
            bias[n] = b[col];
        }
    dst.kin = kin;
    if (decoder) if (int rc = pack_persist(m, dst, wt, bias, Kt)) return rc;
    if (int rc = upload(dst.wt, wt)) return rc;
    return upload(dst.bias, bias);
}

// Decoder layer 1 with the input embedding folded in: (p.E).K = p.(E.K) (seq2seq.py:319 feeds the layer
// with char_input_proj(p)), so the step needs no separate embedding GEMM and the layer's contraction
// shrinks from W+W to Vp+W.  E.K is formed in float64 and rounded once.  Rows [0,Vp) of the fused weight
// take the fed-back distribution, then (top cell only) the context rows, then the recurrent rows.
static int pack_dec1(casv_model* m, LstmW& dst, const std::string& prefix, int kextra) {
    const int W = m->W, V = m->V, Vp = m->Vp, Kt = Vp + kextra + W;
    const auto& E = m->host["E"];
    const auto& K = m->host[prefix + "_K"]; const auto& R = m->host[prefix + "_R"]; const auto& b = m->host[prefix + "_b"];
    std::vector<double> ek((size_t)V * 4 * W, 0.0);
    for (int v = 0; v < V; ++v)
        for (int k = 0; k < W; ++k) {
            const double e = E[(size_t)v * W + k];
            const float* krow = &K[(size_t)k * 4 * W];
            double* out = &ek[(size_t)v * 4 * W];
            for (int c = 0; c < 4 * W; ++c) out[c] += e * (double)krow[c];
        }
    std::vector<float> wt((size_t)4 * W * Kt, 0.f), bias(4 * W);
    for (int u = 0; u < W; ++u)
        for (int g = 0; g < 4; ++g) {
            const int n = (u / 32) * 128 + g * 32 + (u % 32), col = g * W + u;
            float* row = &wt[(size_t)n * Kt];
            for (int v = 0; v < V; ++v) row[v] = (float)ek[(size_t)v * 4 * W + col];
            for (int k = 0; k < kextra; ++k) row[Vp + k] = K[(size_t)(W + k) * 4 * W + col];
            for (int k = 0; k < W; ++k) row[Vp + kextra + k] = R[(size_t)k * 4 * W + col];
            bias[n] = b[col];
        }
    dst.kin = Vp + kextra;
    if (int rc = pack_persist(m, dst, wt, bias, Kt)) return rc;
    if (int rc = upload(dst.wt, wt)) return rc;
    return upload(dst.bias, bias);
}

extern "C" int casv_commit_weights(casv_model* m) {
    if (!m) return fail(CASV_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(m->device));
    for (auto& l : m->dec) gemm_split_invalidate(l.wt.as<float>());          // (split arithmetic: images of the old weights)
    gemm_split_invalidate(m->WaT.as<float>()); gemm_split_invalidate(m->E.as<float>());
    m->enc_tab_ready = false;           // (layer 1's per-character table is a function of E and the layer's kernels: rebuilt on its next use)
    for (auto& kv : m->expect)
        if (!m->host.count(kv.first)) return fail(CASV_ERR_STATE, "weight '%s' has not been set", kv.first.c_str());
    const int W = m->W, C = m->C, D = m->D;
    const auto& E = m->host["E"];
    if (int rc = upload(m->E, E)) return rc;
    if (int rc = pack_lstm(m, m->enc_fw, "enc1_fw", W, true)) return rc;
    if (int rc = pack_lstm(m, m->enc_bw, "enc1_bw", W, true)) return rc;
    const bool deep = m->cfg.deep_bidirectional_encoder != 0;
    for (int n = 2; n <= D && !deep; ++n) if (int rc = pack_lstm(m, m->enc[n], "enc" + std::to_string(n), n == 2 ? 2 * W : W, true)) return rc;
    for (int n = 2; n <= D && deep; ++n) {
        if (int rc = pack_lstm(m, m->enc_dfw[n], "enc" + std::to_string(n) + "_fw", 2 * W)) return rc;
        if (int rc = pack_lstm(m, m->enc_dbw[n], "enc" + std::to_string(n) + "_bw", 2 * W)) return rc;
    }
    if (D == 1) {
        if (int rc = pack_dec1(m, m->dec[1], "dec1", C)) return rc;
    } else {
        if (int rc = pack_dec1(m, m->dec[1], "dec1", 0)) return rc;
        for (int n = 2; n < D; ++n) if (int rc = pack_lstm(m, m->dec[n], "dec" + std::to_string(n), W, true)) return rc;
        if (int rc = pack_lstm(m, m->dec[D], "dec" + std::to_string(D), W + C, true)) return rc;
    }
    const auto& Wa = m->host["att_Wa"]; const auto& U = m->host["att_U"];
    std::vector<float> wat((size_t)W * W), ut((size_t)W * C);
    for (int j = 0; j < W; ++j) for (int k = 0; k < W; ++k) wat[(size_t)j * W + k] = Wa[(size_t)k * W + j];
    for (int j = 0; j < W; ++j) for (int c = 0; c < C; ++c) ut[(size_t)j * C + c] = U[(size_t)c * W + j];
    if (int rc = upload(m->WaT, wat)) return rc;
    if (int rc = upload(m->UT, ut)) return rc;
    {   // the persistent decoder's copies: K permuted per 16-tile, output rows padded to Vp with zeros
        const int V = m->V, Vp = m->Vp;
        std::vector<float> wap((size_t)W * W), ep((size_t)Vp * W, 0.f);
        for (int j = 0; j < W; ++j) persist_permute_row(&wat[(size_t)j * W], &wap[(size_t)j * W], W);
        for (int v = 0; v < V; ++v) persist_permute_row(&E[(size_t)v * W], &ep[(size_t)v * W], W);
        if (int rc = upload(m->WaP, wap)) return rc;
        if (int rc = upload(m->EP, ep)) return rc;
    }
    if (int rc = upload(m->bUW, m->host["att_bUW"])) return rc;
    if (int rc = upload(m->va, m->host["att_va"])) return rc;
    if (int rc = upload(m->bv, m->host["att_bv"])) return rc;
    if (m->cfg.bridge_dense)
        for (int n = 1; n <= D; ++n)
            for (int s = 0; s < 2; ++s) {
                const std::string b = "bridge" + std::to_string(n) + (s ? "_c" : "_h");
                const auto& K = m->host[b + "_K"];
                std::vector<float> kt((size_t)W * W);           // Bt[j][k] = K[k][j]
                for (int j = 0; j < W; ++j) for (int k = 0; k < W; ++k) kt[(size_t)j * W + k] = K[(size_t)k * W + j];
                if (int rc = upload(s ? m->br_cT[n] : m->br_hT[n], kt)) return rc;
                if (int rc = upload(s ? m->br_cb[n] : m->br_hb[n], m->host[b + "_b"])) return rc;
            }
    m->committed = true;
    ++m->commit_gen;                    // (a scoring state built from the weights before is rebuilt: score.hip, score_state)
    return CASV_OK;
}

// ---- result records on the device (multi-GPU gather) ----
extern "C" int casv_records_reset(casv_model* m, int32_t rows, int32_t S) {
    if (!m) return fail(CASV_ERR_ARG, "null argument");
    if (rows < 1 || S < 1 || S > 2 * CASV_MAX_T) return fail(CASV_ERR_ARG, "bad record buffer shape rows=%d S=%d", rows, S);
    HIPCHK(hipSetDevice(m->device));
    const size_t bytes = (size_t)rows * (2 * S + 4) * 4;
    if (int rc = m->rec.ensure(bytes)) return rc;
    HIPCHK(hipMemsetAsync(m->rec.p, 0, bytes, m->stream));
    m->rec_rows = rows; m->rec_S = S;
    return CASV_OK;
}

extern "C" int casv_records_append(casv_model* m, int32_t row_offset) {
    if (!m) return fail(CASV_ERR_ARG, "null argument");
    if (!m->rec.p || !m->rec_rows) return fail(CASV_ERR_STATE, "casv_records_reset first");
    if (!m->last_decode) return fail(CASV_ERR_STATE, "no decode call to take results from");
    if (m->last_signature != decode_buffers_signature(m)) { m->last_decode = 0; return fail(CASV_ERR_STATE, "the decode results have been released"); }
    if (m->last_S != m->rec_S) return fail(CASV_ERR_ARG, "the last decode ran %d steps, the record buffer holds %d", m->last_S, m->rec_S);
    const int B = m->B;
    if (row_offset < 0 || row_offset + B > m->rec_rows) return fail(CASV_ERR_ARG, "rows [%d, %d) outside the record buffer of %d rows", row_offset, row_offset + B, m->rec_rows);
    HIPCHK(hipSetDevice(m->device));
    RecordSrc r{};
    r.B = B; r.S = m->last_S; r.T = m->T; r.A = m->A; r.eos = m->eos;
    r.src_idx = m->d_idx.as<int>(); r.src_val = m->d_val.as<float>();
    // (casv_set_encoder_outputs leaves d_idx / d_val alone: they would still hold the batch of an earlier casv_encode, read with
    // this batch's B and T -- wrong padding decisions and fallback characters, beyond the allocation if this batch is larger)
    if (!r.src_idx || m->A < 1 || m->enc_explicit)
        return fail(CASV_ERR_STATE, "records need the input lines: the last decode's encoder outputs were handed in (casv_set_encoder_outputs), not computed by casv_encode");
    if (m->last_decode == 2) {
        r.idx = m->bo_idx.as<int>(); r.prob = m->bo_prob.as<float>(); r.len = m->bo_len.as<int>(); r.score = m->bo_score.as<double>();
        r.row_mul = m->last_rows / B;                   // max_results rows per line, best first
    } else {
        if (m->last_mode != 0) return fail(CASV_ERR_STATE, "records are defined for the batched greedy mode (0) and the beam");
        r.idx = m->o_idx.as<int>(); r.prob = m->o_prob.as<float>(); r.len = nullptr; r.score = nullptr; r.row_mul = 1;
    }
    launch_pack_records(r, m->rec.as<int>() + (size_t)row_offset * (2 * m->rec_S + 4), m->stream);
    HIPCHK(hipGetLastError());
    return CASV_OK;
}

extern "C" int casv_records_device_ptr(casv_model* m, void** ptr, int64_t* bytes) {
    if (!m || !ptr) return fail(CASV_ERR_ARG, "null argument");
    if (!m->rec.p || !m->rec_rows) return fail(CASV_ERR_STATE, "casv_records_reset first");
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipStreamSynchronize(m->stream));            // whoever reads through the pointer uses another stream
    *ptr = m->rec.p;
    if (bytes) *bytes = (int64_t)m->rec_rows * (2 * m->rec_S + 4) * 4;
    return CASV_OK;
}

extern "C" int casv_records_read(casv_model* m, int32_t* out) {
    if (!m || !out) return fail(CASV_ERR_ARG, "null argument");
    if (!m->rec.p || !m->rec_rows) return fail(CASV_ERR_STATE, "casv_records_reset first");
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipMemcpyAsync(out, m->rec.p, (size_t)m->rec_rows * (2 * m->rec_S + 4) * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}

extern "C" int casv_get_stat(casv_model* m, const char* key, int64_t* value) {
    if (!m || !key || !value) return fail(CASV_ERR_ARG, "null argument");
    if (!strcmp(key, "beam_max_new_keys")) { *value = m->stat_beam[0]; return CASV_OK; }
    if (!strcmp(key, "beam_sort_capacity")) { *value = 4096; return CASV_OK; }
    if (!strcmp(key, "cus")) { *value = m->ncu; return CASV_OK; }
    if (!strcmp(key, "encoder_persistent")) { *value = m->stat_enc_persistent; return CASV_OK; }
    if (!strcmp(key, "encoder_table")) { *value = m->stat_enc_table; return CASV_OK; }
    if (!strcmp(key, "encoder_ahead")) { *value = m->stat_enc_ahead; return CASV_OK; }
    if (!strcmp(key, "encoder_table_builds")) { *value = m->stat_enc_table_builds; return CASV_OK; }
    if (!strcmp(key, "decoder_persistent")) { *value = m->stat_dec_persistent; return CASV_OK; }
    if (!strcmp(key, "decode_give_ups")) { *value = m->stat_decode_give_ups; return CASV_OK; }
    if (!strcmp(key, "decoder_persist_per_cu")) { *value = m->stat_dec_plan[0]; return CASV_OK; }
    if (!strcmp(key, "decoder_persist_g_lstm")) { *value = m->stat_dec_plan[1]; return CASV_OK; }
    if (!strcmp(key, "decoder_persist_g_att")) { *value = m->stat_dec_plan[2]; return CASV_OK; }
    if (!strcmp(key, "decoder_persist_g_plain")) { *value = m->stat_dec_plan[3]; return CASV_OK; }
    if (!strcmp(key, "encoder_persist_per_cu")) { *value = m->stat_enc_plan[0]; return CASV_OK; }
    if (!strcmp(key, "encoder_persist_grid")) { *value = m->stat_enc_plan[1]; return CASV_OK; }
    if (!strcmp(key, "train_persistent_launches")) { *value = m->stat_train_launches; return CASV_OK; }
    if (!strcmp(key, "train_give_ups")) { *value = m->stat_train_give_ups; return CASV_OK; }
    if (!strcmp(key, "gemm_jobs_forms")) { *value = m->stat_jobs[0]; return CASV_OK; }
    if (!strcmp(key, "gemm_jobs_launches")) { *value = m->stat_jobs[1]; return CASV_OK; }
    if (!strcmp(key, "gemm_jobs_shares")) { *value = m->stat_jobs[2]; return CASV_OK; }
    if (!strcmp(key, "bwd_step_shares")) { *value = m->stat_bwd_step[0]; return CASV_OK; }
    if (!strcmp(key, "bwd_step_groups")) { *value = m->stat_bwd_step[1]; return CASV_OK; }
    if (!strcmp(key, "tn_split")) { *value = m->stat_tn[0]; return CASV_OK; }
    if (!strcmp(key, "tn_shares")) { *value = m->stat_tn[1]; return CASV_OK; }
    if (!strcmp(key, "tn_nonempty_shares")) { *value = m->stat_tn[2]; return CASV_OK; }
    if (!strcmp(key, "sample_cut_rows")) { *value = m->stat_sample_cut_rows; return CASV_OK; }
    if (!strcmp(key, "align_rounds")) { *value = m->stat_align_rounds; return CASV_OK; }
    if (!strcmp(key, "align_fill_ticks")) { *value = m->stat_align_ticks[0]; return CASV_OK; }
    if (!strcmp(key, "align_walk_ticks")) { *value = m->stat_align_ticks[1]; return CASV_OK; }
    return fail(CASV_ERR_ARG, "unknown statistic '%s'", key);
}

extern "C" int casv_profile(casv_model* m, int32_t enable) {
    if (!m) return fail(CASV_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->prof.reset();
    m->prof.on = enable != 0;
    m->prof.only_lstm = enable == 2 || enable == 3;
    m->prof.sample = enable == 3 ? 13 : 1;       // (13: coprime to the layers of a step, every layer is sampled equally often)
    m->prof.seen = 0;
    return CASV_OK;
}

extern "C" int casv_profile_read(casv_model* m, const char* name, int64_t* launches, double* total_ms, double* flops,
                                 double* bytes) {
    if (!m || !name) return fail(CASV_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->prof.collect();
    for (int i = 0; i < PC_COUNT; ++i)
        if (!strcmp(name, kProfNames[i])) {
            if (launches) *launches = m->prof.launches[i];
            if (total_ms) *total_ms = m->prof.ms[i];
            if (flops) *flops = m->prof.flops[i];
            if (bytes) *bytes = m->prof.bytes[i];
            return CASV_OK;
        }
    return fail(CASV_ERR_ARG, "unknown kernel class '%s'", name);
}

// Measurement aid: time `iters` launches of one GEMM shape in isolation (random operands).
extern "C" int casv_debug_gemm(casv_model* m, int32_t lstm, int32_t M, int32_t N, int32_t K, int32_t gather,
                               int32_t iters, double* ms_per_launch) {
    if (!m || !ms_per_launch) return fail(CASV_ERR_ARG, "null argument");
    if (K % 32 || (lstm && N % 128)) return fail(CASV_ERR_ARG, "K must be a multiple of 32 (and N of 128 for lstm)");
    HIPCHK(hipSetDevice(m->device));
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_CHAIN));
    DevBuf A, Bt, bias, C, cst, rows;
    DebugBuffers release_on_exit{m->stream, &Bt};
    if (int rc = A.ensure((size_t)M * K * 4)) return rc;
    if (int rc = Bt.ensure((size_t)N * K * 4)) return rc;
    if (int rc = bias.ensure((size_t)N * 4)) return rc;
    if (int rc = C.ensure((size_t)M * N * 4)) return rc;
    if (int rc = cst.ensure((size_t)M * N * 4)) return rc;
    if (int rc = rows.ensure((size_t)M * 4)) return rc;
    std::vector<float> h((size_t)std::max((size_t)M, (size_t)N) * K);
    unsigned s = 12345u;
    for (auto& v : h) { s = s * 1664525u + 1013904223u; v = ((s >> 8) & 0xffff) / 65536.0f - 0.5f; }
    HIPCHK(hipMemcpy(A.p, h.data(), (size_t)M * K * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(Bt.p, h.data(), (size_t)N * K * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(bias.p, 0, (size_t)N * 4));
    HIPCHK(hipMemset(cst.p, 0, (size_t)M * N * 4));
    std::vector<int> hr(M);
    for (int i = 0; i < M; ++i) hr[i] = gather ? (int)(((long long)i * 7919) % M) : i;
    HIPCHK(hipMemcpy(rows.p, hr.data(), (size_t)M * 4, hipMemcpyHostToDevice));
    GemmArgs g{};
    g.nseg = 1; g.a[0] = mkseg(A.as<float>(), K, K, 0, rows.as<int>());
    g.Bt = Bt.as<float>(); g.bias = bias.as<float>(); g.M = M; g.N = N; g.Ktot = K;
    g.b_static = 1;         // (split arithmetic: as the decoder's weights; the image is dropped again below)
    g.out = mkslot(C.as<float>(), lstm ? N / 4 : N);
    if (lstm) { g.c_in = mkseg(cst.as<float>(), N / 4, N / 4, 0, rows.as<int>()); g.c_out = mkslot(cst.as<float>() + (size_t)M * N / 2, N / 4); }
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) launch_gemm(m->gemm, lstm ? EPI_LSTM : EPI_PLAIN, g, m->stream);
    HIPCHK(hipEventRecord(e0, m->stream));
    for (int i = 0; i < iters; ++i) launch_gemm(m->gemm, lstm ? EPI_LSTM : EPI_PLAIN, g, m->stream);
    HIPCHK(hipEventRecord(e1, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    float t = 0; HIPCHK(hipEventElapsedTime(&t, e0, e1));
    *ms_per_launch = t / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
#ifdef CASV_S2_CLOCK
    s2_clock_dump();
#endif
    return CASV_OK;
}

// Test support: ONE plain contraction on the caller's operands through the library's launcher (whatever tile shape, split-K form
// and arithmetic the options select), result back to the host.
extern "C" int casv_debug_contract(casv_model* m, int32_t flags, int32_t M, int32_t N, int32_t K, const float* A_, const float* Bt_,
                                   const float* bias_, float* C_) {
    if (!m || !A_ || !Bt_ || !C_) return fail(CASV_ERR_ARG, "null argument");
    if (M < 1 || N < 1 || K < 32 || K % 32) return fail(CASV_ERR_ARG, "M, N positive, K a positive multiple of 32");
    HIPCHK(hipSetDevice(m->device));
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_CHAIN));
    DevBuf A, Bt, bias, C;
    DebugBuffers release_on_exit{m->stream, &Bt};
    if (int rc = A.ensure((size_t)M * K * 4)) return rc;
    if (int rc = Bt.ensure((size_t)N * K * 4)) return rc;
    if (int rc = bias.ensure((size_t)N * 4)) return rc;
    if (int rc = C.ensure((size_t)M * N * 4)) return rc;
    HIPCHK(hipMemcpyAsync(A.p, A_, (size_t)M * K * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(Bt.p, Bt_, (size_t)N * K * 4, hipMemcpyHostToDevice, m->stream));
    if (bias_) HIPCHK(hipMemcpyAsync(bias.p, bias_, (size_t)N * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemsetAsync(C.p, 0xff, (size_t)M * N * 4, m->stream));           // (NaN: an element the launch does not write shows)
    if (flags & 8) {
        // K-major operands (the train step's weight gradients): A_ is [K][M], Bt_ is [K][N], C = A^T . B (+ colsum(A) into bias_'s place:
        // not taken here) through gemm_tn_split.hip under the split arithmetic where the shape has that form, else gemm_tn.hip
        if (M % 4 || N % 4) return fail(CASV_ERR_ARG, "K-major operands: M and N multiples of 4");
        TnArgs t{};
        t.A = A.as<float>(); t.lda = M; t.B = Bt.as<float>(); t.ldb = N; t.C = C.as<float>(); t.ldc = N;
        t.M = M; t.Mstore = M; t.N = N; t.K = K; t.accumulate = 0; t.out_zeroed = 0; t.colsum = nullptr;
        (void)launch_gemm_tn_any(m->gemm, t, nullptr, m->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(C_, C.p, (size_t)M * N * 4, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
        return CASV_OK;
    }
    GemmArgs g{};
    g.nseg = 1; g.a[0] = mkseg(A.as<float>(), K, K, 0);
    g.Bt = Bt.as<float>(); g.bias = bias_ ? bias.as<float>() : nullptr; g.M = M; g.N = N; g.Ktot = K;
    g.out = mkslot(C.as<float>(), N);
    if (flags & 1) g.ksplit = -1;               // the launcher may split K over workgroups (train step's plain contractions)
    if (flags & 2) g.kgroups = 2;               // ... and over two wave groups of a workgroup
    if (flags & 4) g.b_static = 1;              // Bt is a weight: the split-bf16 arithmetic may keep a pre-split image of it
    launch_gemm(m->gemm, EPI_PLAIN, g, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(C_, C.p, (size_t)M * N * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}

// Test support: ONE weight-gradient contraction C[m][n] (+)= sum_k A[k][m] * B[k][n] (m < Mstore) through the train step's own
// dispatch (launch_gemm_tn_any, under the train step's arithmetic), on operands copied in with their strides.  Rows Mstore..M-1 of C
// and colsum get a guard pattern on the device: a launch that stores there is an error.
extern "C" int casv_debug_contract_tn(casv_model* m, int32_t flags, int32_t M, int32_t Mstore, int32_t N, int32_t K,
                                      const float* A_, int64_t lda, const float* B_, int64_t ldb, float* C_, int64_t ldc,
                                      float* colsum_) {
    if (!m || !A_ || !B_ || !C_ || ((flags & 2) && !colsum_)) return fail(CASV_ERR_ARG, "null argument");
    if (flags & ~7) return fail(CASV_ERR_ARG, "flags: 1 accumulate, 2 colsum, 4 ordered form");
    if (M < 4 || N < 4 || K < 1 || M % 4 || N % 4 || Mstore < 1 || Mstore > M)
        return fail(CASV_ERR_ARG, "M and N positive multiples of 4, 1 <= Mstore <= M, K positive");
    if (lda < M || ldb < N || ldc < N || lda % 4 || ldb % 4) return fail(CASV_ERR_ARG, "lda >= M, ldb >= N (multiples of 4), ldc >= N");
    HIPCHK(hipSetDevice(m->device));
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_TRAIN));
    const size_t na = (size_t)(K - 1) * lda + M, nb = (size_t)(K - 1) * ldb + N;
    const size_t nc = (size_t)(Mstore - 1) * ldc + N, nc_all = (size_t)M * ldc + N;      // (guard: every row of M and one more)
    DevBuf A, B, C, cs, ws;
    DebugBuffers release_on_exit{m->stream};
    if (int rc = A.ensure(na * 4)) return rc;
    if (int rc = B.ensure(nb * 4)) return rc;
    if (int rc = C.ensure(nc_all * 4)) return rc;
    if (int rc = cs.ensure((size_t)(M + 1) * 4)) return rc;
    HIPCHK(hipMemcpyAsync(A.p, A_, na * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(B.p, B_, nb * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemsetAsync(C.p, 0xff, nc_all * 4, m->stream));
    HIPCHK(hipMemcpyAsync(C.p, C_, nc * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemsetAsync(cs.p, 0xff, (size_t)(M + 1) * 4, m->stream));
    if (flags & 2) HIPCHK(hipMemcpyAsync(cs.p, colsum_, (size_t)Mstore * 4, hipMemcpyHostToDevice, m->stream));
    TnArgs t{};
    t.A = A.as<float>(); t.lda = lda; t.B = B.as<float>(); t.ldb = ldb; t.C = C.as<float>(); t.ldc = ldc;
    t.M = M; t.Mstore = Mstore; t.N = N; t.K = K; t.accumulate = flags & 1; t.out_zeroed = 0;
    t.colsum = (flags & 2) ? cs.as<float>() : nullptr;
    float* wsp = nullptr;
    if (flags & 4) {
        if (int rc = ws.ensure(gemm_tn_ordered_floats(m->gemm, t) * 4)) return rc;
        wsp = ws.as<float>();
    }
    const TnLaunch r = launch_gemm_tn_any(m->gemm, t, wsp, m->stream);
    HIPCHK(hipGetLastError());
    m->stat_tn[0] = r.split; m->stat_tn[1] = r.shares; m->stat_tn[2] = r.nonempty;
    std::vector<uint32_t> guard(nc_all - nc), cguard((size_t)(M + 1 - Mstore));
    HIPCHK(hipMemcpyAsync(C_, C.p, nc * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(guard.data(), C.as<float>() + nc, guard.size() * 4, hipMemcpyDeviceToHost, m->stream));
    if (flags & 2) HIPCHK(hipMemcpyAsync(colsum_, cs.p, (size_t)Mstore * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(cguard.data(), cs.as<float>() + Mstore, cguard.size() * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    for (uint32_t v : guard) if (v != 0xffffffffu) return fail(CASV_ERR_STATE, "the launch stored past row Mstore - 1 of C");
    for (uint32_t v : cguard) if (v != 0xffffffffu) return fail(CASV_ERR_STATE, "the launch stored past colsum[Mstore - 1]");
    return CASV_OK;
}

// Test support: one batch of forward jobs with the whole operand machinery of gemm_args.h, on host data (casv_debug_gemm_jobs).
// Nothing is launched unless every address a kernel can form from the arguments lies inside a buffer allocated here: the kernels
// clamp rows to M - 1 and columns to N - 1, read [0, width) of a row, rows[m] for every m < M (live or not), the cell state's N / 4
// units, nact[line] for every line of the job; they store rows < M only.
namespace {
constexpr long long DEBUG_JOBS_MAX_FLOATS = 1LL << 28;      // per buffer (1 GiB)
// the slot a step selects; false: outside [0, slots)
bool debug_slot_ok(int step, int mul, int add, int slots) {
    const long long s = (long long)step * mul + add;
    return s >= 0 && s < slots;
}
// an input part of job j (K segment, cell state, zinit) at every step of `steps`
int check_debug_rows(const casv_debug_rows& r, const char* what, int j, int M, const int* steps, int nsteps) {
    if (!r.pool) return fail(CASV_ERR_ARG, "job %d %s: no pool", j, what);
    if (r.slots < 1 || r.slots > 64 || r.pool_rows < 1 || r.width < 1 || r.ld < r.width || r.ld % 4 || r.ld > (1 << 16))
        return fail(CASV_ERR_ARG, "job %d %s: slots in [1, 64], pool_rows >= 1, ld >= width >= 1, ld a multiple of 4", j, what);
    if ((long long)r.slots * r.pool_rows * r.ld > DEBUG_JOBS_MAX_FLOATS) return fail(CASV_ERR_ARG, "job %d %s: pool too large", j, what);
    if (std::abs((long long)r.step_mul) > 64 || std::abs((long long)r.step_add) > 4096) return fail(CASV_ERR_ARG, "job %d %s: step_mul / step_add out of range", j, what);
    if (r.skip_first != 0 && r.skip_first != 1) return fail(CASV_ERR_ARG, "job %d %s: skip_first is 0 or 1", j, what);
    if (r.rows) { for (int m = 0; m < M; ++m) if (r.rows[m] < 0 || r.rows[m] >= r.pool_rows) return fail(CASV_ERR_ARG, "job %d %s: rows[%d] = %d outside [0, %d)", j, what, m, r.rows[m], r.pool_rows); }
    else if (r.pool_rows < M) return fail(CASV_ERR_ARG, "job %d %s: %d pool rows for %d ungathered rows", j, what, r.pool_rows, M);
    for (int i = 0; i < nsteps; ++i) {
        if (steps[i] == 0 && (r.skip_first || r.first)) continue;         // (the pool is not read at step 0)
        if (!debug_slot_ok(steps[i], r.step_mul, r.step_add, r.slots)) return fail(CASV_ERR_ARG, "job %d %s: step %d selects a slot outside [0, %d)", j, what, steps[i], r.slots);
    }
    return CASV_OK;
}
int check_debug_out(const casv_debug_out& o, const char* what, int j, int M, int width, const int* steps, int nsteps) {
    if (!o.data) return fail(CASV_ERR_ARG, "job %d %s: no data", j, what);
    if (o.slots < 1 || o.slots > 64 || o.ld < width || o.ld % 4 || o.ld > (1 << 16)) return fail(CASV_ERR_ARG, "job %d %s: slots in [1, 64], ld >= %d and a multiple of 4", j, what, width);
    if (((long long)o.slots * M + 1) * o.ld > DEBUG_JOBS_MAX_FLOATS) return fail(CASV_ERR_ARG, "job %d %s: too large", j, what);
    if (std::abs((long long)o.step_mul) > 64 || std::abs((long long)o.step_add) > 4096) return fail(CASV_ERR_ARG, "job %d %s: step_mul / step_add out of range", j, what);
    for (int i = 0; i < nsteps; ++i)
        if (!debug_slot_ok(steps[i], o.step_mul, o.step_add, o.slots)) return fail(CASV_ERR_ARG, "job %d %s: step %d selects a slot outside [0, %d)", j, what, steps[i], o.slots);
    return CASV_OK;
}
int check_debug_job(int epi, const casv_debug_job& d, int j, const int* steps, int nsteps, int kmult = 32) {
    const bool lstm = epi == EPI_LSTM && !d.epi_plain;
    if (d.M < 1 || d.M > (1 << 16) || d.N < 1 || d.N > (1 << 14) || d.Ktot < 32 || d.Ktot > (1 << 14) || d.Ktot % 4 || d.nseg < 1 || d.nseg > 3)
        return fail(CASV_ERR_ARG, "job %d: M in [1, 65536], N in [1, 16384], Ktot in [32, 16384] and a multiple of 4, 1..3 segments", j);
    if (lstm && d.N % 128) return fail(CASV_ERR_ARG, "job %d: N must be a multiple of 128 for the LSTM epilogue", j);
    if (!d.Bt) return fail(CASV_ERR_ARG, "job %d: no Bt", j);
    if ((d.b_static != 0 && d.b_static != 1) || (d.epi_plain != 0 && d.epi_plain != 1)) return fail(CASV_ERR_ARG, "job %d: b_static and epi_plain are 0 or 1", j);
    long long wsum = 0;
    for (int i = 0; i < d.nseg; ++i) {
        const casv_debug_rows& r = d.a[i];
        const std::string what = "segment " + std::to_string(i);
        if (int rc = check_debug_rows(r, what.c_str(), j, d.M, steps, nsteps)) return rc;
        if (r.width % kmult) return fail(CASV_ERR_ARG, "job %d %s: width %d is no multiple of %d", j, what.c_str(), r.width, kmult);
        if (r.koff < 0 || r.koff % 4 || (long long)r.koff + r.width > d.Ktot) return fail(CASV_ERR_ARG, "job %d %s: koff a non-negative multiple of 4, koff + width <= Ktot", j, what.c_str());
        wsum += r.width;
    }
    if (wsum > d.Ktot) return fail(CASV_ERR_ARG, "job %d: the segments' widths sum to %lld > Ktot = %d", j, wsum, d.Ktot);
    if (int rc = check_debug_out(d.out, "out", j, d.M, lstm ? d.N / 4 : d.N, steps, nsteps)) return rc;
    if (lstm) {
        if (int rc = check_debug_rows(d.c_in, "c_in", j, d.M, steps, nsteps)) return rc;
        if (d.c_in.width != d.N / 4) return fail(CASV_ERR_ARG, "job %d c_in: width must be N / 4", j);
        if (int rc = check_debug_out(d.c_out, "c_out", j, d.M, d.N / 4, steps, nsteps)) return rc;
        if (d.zinit.pool) {
            if (int rc = check_debug_rows(d.zinit, "zinit", j, d.M, steps, nsteps)) return rc;
            if (d.zinit.width != d.N || d.zinit.pool_rows != d.M || d.zinit.rows || d.zinit.first || d.zinit.skip_first)
                return fail(CASV_ERR_ARG, "job %d zinit: width = N, pool_rows = M, no rows / first / skip_first", j);
        }
        if (d.gates_out.data) if (int rc = check_debug_out(d.gates_out, "gates_out", j, d.M, d.N, steps, nsteps)) return rc;
        if (d.out2.data) if (int rc = check_debug_out(d.out2, "out2", j, d.M, d.N / 4, steps, nsteps)) return rc;
    } else if (d.zinit.pool || d.gates_out.data || d.out2.data || d.c_out.data) {
        return fail(CASV_ERR_ARG, "job %d: c_out, zinit, gates_out and out2 belong to LSTM jobs", j);
    }
    if (d.nact) {
        if (d.nact_group < 1 || d.nact_lines != (d.M + d.nact_group - 1) / d.nact_group) return fail(CASV_ERR_ARG, "job %d: nact needs nact_group >= 1 and one entry per line", j);
        for (int l = 0; l < d.nact_lines; ++l) if (d.nact[l] < 0 || d.nact[l] > d.nact_group) return fail(CASV_ERR_ARG, "job %d: nact[%d] outside [0, nact_group]", j, l);
    }
    return CASV_OK;
}
// the train step's launch fields of job j (casv_debug_gemm_jobs_sum): plain_gemm()'s, on plain-epilogue jobs of a plain batch only
int check_debug_sum(int epi, const casv_debug_job& d, const casv_debug_sum& s, int j, int step_by_ptr) {
    if (s.ksplit < -1 || s.ksplit > 64 || (s.kgroups != 0 && s.kgroups != 2) || (s.accumulate != 0 && s.accumulate != 1) || (s.out_zeroed != 0 && s.out_zeroed != 1))
        return fail(CASV_ERR_ARG, "job %d: ksplit in [-1, 64], kgroups 0 or 2, accumulate and out_zeroed 0 or 1", j);
    const bool any = s.ksplit || s.kgroups || s.accumulate || s.out_zeroed;
    if (any && (epi != EPI_PLAIN || d.epi_plain)) return fail(CASV_ERR_ARG, "job %d: ksplit, kgroups, accumulate and out_zeroed belong to the plain-epilogue jobs of an epi = 0 batch", j);
    if (s.ksplit != 0 && step_by_ptr) return fail(CASV_ERR_ARG, "job %d: a job that asks for split-K cannot take its step from a device word", j);
    if (s.accumulate && s.out_zeroed) return fail(CASV_ERR_ARG, "job %d: accumulate and out_zeroed exclude each other", j);
    return CASV_OK;
}
}  // namespace

// (`acc`: casv_debug_gemm_jobs_acc -- per job an accumulator input, pool == NULL: none; `sums`: casv_debug_gemm_jobs_sum -- per job the
// train step's launch fields, under ordered sums if `ordered`)
static int debug_gemm_jobs(casv_model* m, int32_t epi, int32_t count, const casv_debug_job* jobs, const casv_debug_rows* acc, int32_t step, int32_t step_by_ptr,
                           const casv_debug_sum* sums = nullptr, int32_t ordered = 0) {
    if (!m || !jobs) return fail(CASV_ERR_ARG, "null argument");
    if ((epi != EPI_PLAIN && epi != EPI_LSTM) || count < 1 || count > GEMM_MAX_JOBS || step < 0 || step > 4096 || (step_by_ptr != 0 && step_by_ptr != 1))
        return fail(CASV_ERR_ARG, "epi 0 / 1, 1..%d jobs, step in [0, 4096], step_by_ptr 0 / 1", GEMM_MAX_JOBS);
    // (a step that arrives through the device word: the arguments' immediate step is 0, and must be harmless if a kernel took it)
    const int steps[2] = {step, 0};
    const int nsteps = step_by_ptr ? 2 : 1;
    // (the split tiles contract K in tiles of 16: with `acc` the segments may be that narrow, and every form is a split one, below)
    for (int j = 0; j < count; ++j) if (int rc = check_debug_job(epi, jobs[j], j, steps, nsteps, acc ? 16 : 32)) return rc;
    for (int j = 0; j < count && acc; ++j) {
        if (!acc[j].pool) continue;
        if (int rc = check_debug_rows(acc[j], "acc_in", j, jobs[j].M, steps, nsteps)) return rc;
        if (acc[j].width != jobs[j].N || acc[j].first || acc[j].skip_first) return fail(CASV_ERR_ARG, "job %d acc_in: width = N, no first / skip_first", j);
    }
    if (ordered != 0 && ordered != 1) return fail(CASV_ERR_ARG, "ordered is 0 or 1");
    for (int j = 0; j < count && sums; ++j) if (int rc = check_debug_sum(epi, jobs[j], sums[j], j, step_by_ptr)) return rc;
    HIPCHK(hipSetDevice(m->device));
    SplitScope arithmetic(m, arithmetic_of(m, ENTRY_CHAIN));
    OrderedScope ordered_sums(m, ordered != 0);         // (the train step's "deterministic" option: no launch splits K over workgroups)
    if (acc && !m->gemm.arithmetic) return fail(CASV_ERR_ARG, "casv_debug_gemm_jobs_acc needs a split arithmetic (option \"arithmetic\" or \"split_bf16\" = 1 or 2)");
    DebugBuffers dev{m->stream};
    int rc = CASV_OK;
    const int* step_word = nullptr;
    if (step_by_ptr) { step_word = static_cast<const int*>(dev.put(&step, 1, rc)); if (rc) return rc; }
    struct Back { const casv_debug_out* o; float* d; size_t rows; };
    std::vector<Back> back;
    GemmBatch b{};
    b.count = count;
    for (int j = 0; j < count; ++j) {
        const casv_debug_job& d = jobs[j];
        const bool lstm = epi == EPI_LSTM && !d.epi_plain;
        GemmArgs& g = b.g[j];
        auto seg = [&](const casv_debug_rows& r, Seg& s) {
            s = Seg{};
            s.base = static_cast<const float*>(dev.put(r.pool, (size_t)r.slots * r.pool_rows * r.ld, rc)); if (rc) return;
            if (r.rows) { s.rows = static_cast<const int*>(dev.put(r.rows, (size_t)d.M, rc)); if (rc) return; }
            if (r.first) { s.first_base = static_cast<const float*>(dev.put(r.first, (size_t)d.M * r.ld, rc)); if (rc) return; }
            s.slot_stride = (long long)r.pool_rows * r.ld; s.step_mul = r.step_mul; s.step_add = r.step_add;
            s.ld = r.ld; s.width = r.width; s.skip_first = r.skip_first; s.koff = r.koff;
        };
        auto out = [&](const casv_debug_out& o, SlotPtr& p) {
            const size_t rows = (size_t)o.slots * d.M;
            p = SlotPtr{};
            p.base = static_cast<float*>(dev.put(nullptr, (rows + 1) * o.ld, rc)); if (rc) return;      // (one guard row behind the last slot)
            p.slot_stride = (long long)d.M * o.ld; p.step_mul = o.step_mul; p.step_add = o.step_add; p.ld = o.ld;
            back.push_back(Back{&o, p.base, rows});
        };
        g.M = d.M; g.N = d.N; g.Ktot = d.Ktot; g.nseg = d.nseg;
        for (int i = 0; i < d.nseg; ++i) { seg(d.a[i], g.a[i]); if (rc) return rc; }
        g.Bt = static_cast<const float*>(dev.put(d.Bt, (size_t)d.N * d.Ktot, rc)); if (rc) return rc;
        dev.weights.push_back(g.Bt);
        if (d.bias) { g.bias = static_cast<const float*>(dev.put(d.bias, (size_t)d.N, rc)); if (rc) return rc; }
        out(d.out, g.out); if (rc) return rc;
        if (sums) {
            // the addressed slot, rows < M and columns < N: C0 from the host for `accumulate`, zeros for `out_zeroed` (the caller's
            // clear); its pad columns, every other slot and the guard row keep the 0xFF bytes
            const casv_debug_sum& s = sums[j];
            g.ksplit = s.ksplit; g.kgroups = s.kgroups; g.accumulate = s.accumulate; g.out_zeroed = s.out_zeroed;
            const size_t slot = (size_t)((long long)step * d.out.step_mul + d.out.step_add) * d.M * d.out.ld, pitch = (size_t)d.out.ld * 4;
            if (s.accumulate) HIPCHK(hipMemcpy2DAsync(g.out.base + slot, pitch, d.out.data + slot, pitch, (size_t)d.N * 4, d.M, hipMemcpyHostToDevice, m->stream));
            if (s.out_zeroed) HIPCHK(hipMemset2DAsync(g.out.base + slot, pitch, 0, (size_t)d.N * 4, d.M, m->stream));
        }
        if (lstm) {
            seg(d.c_in, g.c_in); if (rc) return rc;
            out(d.c_out, g.c_out); if (rc) return rc;
            if (d.zinit.pool) {
                Seg z; seg(d.zinit, z); if (rc) return rc;
                g.zinit = mkslot(const_cast<float*>(z.base), z.ld, z.slot_stride, z.step_mul, z.step_add);
            }
            if (d.gates_out.data) { out(d.gates_out, g.gates_out); if (rc) return rc; }
            if (d.out2.data) { out(d.out2, g.out2); if (rc) return rc; }
        }
        if (d.nact) { g.nact = static_cast<const int*>(dev.put(d.nact, (size_t)d.nact_lines, rc)); if (rc) return rc; g.nact_group = d.nact_group; }
        g.epi_plain = epi == EPI_LSTM ? d.epi_plain : 0;
        g.b_static = d.b_static;
        g.step_imm = step_by_ptr ? 0 : step; g.step_ptr = step_word;
        if (acc && acc[j].pool) {
            seg(acc[j], g.acc_in); if (rc) return rc;
            g.acc_in.width = 0; g.acc_in.koff = 0;
        }
    }
    // (launch_gemm_batch, keeping the plan that ran for the statistic)
    const GemmPlan planned = plan_gemm_launches(m->gemm, gemm_switches(), epi, b);
    if (!gemm_plan_takes_acc_in(planned)) return fail(CASV_ERR_ARG, "a job with acc_in would not run as 128x128 split tiles");
    const GemmPlan plan = run_gemm_plan(m->gemm, epi, b, planned, m->stream);
    HIPCHK(hipGetLastError());
    m->stat_jobs[0] = 0; m->stat_jobs[1] = plan.count; m->stat_jobs[2] = 0;
    for (int i = 0; i < plan.count; ++i) {
        const GemmLaunchPlan& l = plan.launch[i];
        m->stat_jobs[0] |= 1 << l.form;
        for (int j = 0; j < l.batch.count; ++j) m->stat_jobs[1] += l.clear_jobs >> j & 1;       // (a clear is a launch of its own)
        m->stat_jobs[2] = std::max(m->stat_jobs[2], l.grid_z);
    }
    std::vector<std::vector<uint32_t>> guards(back.size());
    for (size_t i = 0; i < back.size(); ++i) {
        const size_t n = back[i].rows * back[i].o->ld;
        guards[i].resize(back[i].o->ld);
        HIPCHK(hipMemcpyAsync(back[i].o->data, back[i].d, n * 4, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(hipMemcpyAsync(guards[i].data(), back[i].d + n, guards[i].size() * 4, hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    for (const auto& gd : guards) for (uint32_t v : gd) if (v != 0xffffffffu) return fail(CASV_ERR_STATE, "a launch stored past the last row of an output");
    return CASV_OK;
}

extern "C" int casv_debug_gemm_jobs(casv_model* m, int32_t epi, int32_t count, const casv_debug_job* jobs, int32_t step, int32_t step_by_ptr) {
    return debug_gemm_jobs(m, epi, count, jobs, nullptr, step, step_by_ptr);
}
extern "C" int casv_debug_gemm_jobs_acc(casv_model* m, int32_t epi, int32_t count, const casv_debug_job* jobs, const casv_debug_rows* acc,
                                        int32_t step, int32_t step_by_ptr) {
    if (!acc) return fail(CASV_ERR_ARG, "null argument");
    return debug_gemm_jobs(m, epi, count, jobs, acc, step, step_by_ptr);
}
extern "C" int casv_debug_gemm_jobs_sum(casv_model* m, int32_t epi, int32_t count, const casv_debug_job* jobs, const casv_debug_sum* sums,
                                        int32_t ordered, int32_t step, int32_t step_by_ptr) {
    if (!sums) return fail(CASV_ERR_ARG, "null argument");
    return debug_gemm_jobs(m, epi, count, jobs, nullptr, step, step_by_ptr, sums, ordered);
}

extern "C" int casv_debug_activation(casv_model* m, int32_t which, int64_t n, const float* in_, float* out_) {
    if (!m || (n > 0 && (!in_ || !out_))) return fail(CASV_ERR_ARG, "null argument");
    if (which < 0 || which > 2) return fail(CASV_ERR_ARG, "which: 0 tanh, 1 sigmoid, 2 lstm_cell");
    if (n < 0 || n > (1LL << 28)) return fail(CASV_ERR_ARG, "n must be in [0, 2^28]");
    if (n == 0) return CASV_OK;
    HIPCHK(hipSetDevice(m->device));
    const size_t nin = (size_t)n * (which == 2 ? 5 : 1), nout = (size_t)n * (which == 2 ? 2 : 1);
    DevBuf in, out;
    DebugBuffers release_on_exit{m->stream};
    if (int rc = in.ensure(nin * 4)) return rc;
    if (int rc = out.ensure(nout * 4)) return rc;
    HIPCHK(hipMemcpyAsync(in.p, in_, nin * 4, hipMemcpyHostToDevice, m->stream));
    launch_debug_activation(which, in.as<float>(), out.as<float>(), n, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_, out.p, nout * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}

extern "C" int casv_set_option(casv_model* m, const char* key, int64_t value) {
    if (!m || !key) return fail(CASV_ERR_ARG, "null argument");
    if (!strcmp(key, "graph")) { m->use_graph = value != 0; return CASV_OK; }
    if (!strcmp(key, "persistent")) {
        // (2: as -1, and in the train step's first persistent recurrence one workgroup leaves without handing on: its peers give up
        // after their bounded wait and the step falls back to per-step launches -- a test of that path)
        // The fault injection is not part of the production interface: only a process started with CASV_FAULT_INJECTION=1 gets it.
        static const bool fault_ok = [] { const char* e = getenv("CASV_FAULT_INJECTION"); return e && e[0] == '1'; }();
        // (3: as 1, and one workgroup of the split persistent encoder leaves without handing on -- the same test of the encoder's give-up path)
        if (value < -1 || value > (fault_ok ? 3 : 1)) return fail(CASV_ERR_ARG, "persistent must be -1 (by batch size), 0 (per-step kernels) or 1 (always)");
        m->persist_fault_split = value == 3;
        m->persist_mode = value == 3 ? 1 : (int)value; return CASV_OK;
    }
    if (!strcmp(key, "eos")) {
        if (value < 0 || value >= m->V) return fail(CASV_ERR_ARG, "eos index %lld outside the vocabulary", (long long)value);
        m->eos = (int)value; return CASV_OK;
    }
    if (!strcmp(key, "pin_limit_mb")) {
        if (value < 0 || value > 4096) return fail(CASV_ERR_ARG, "pin_limit_mb out of range 0..4096");
        m->pin_limit = (size_t)value << 20; return CASV_OK;
    }
    if (!strcmp(key, "fused_backward")) { m->fused_backward = value != 0; return CASV_OK; }
    if (!strcmp(key, "deterministic")) {        // train step: bits a function of its inputs alone (train.hip)
        if (value < 0 || value > 1) return fail(CASV_ERR_ARG, "deterministic must be 0 or 1");
        m->deterministic = value != 0; return CASV_OK;
    }
    if (!strcmp(key, "lm_predict")) {           // beam decode: children's costs from the LM output
        if (value < 0 || value > 1) return fail(CASV_ERR_ARG, "lm_predict must be 0 or 1");
        m->lm_predict = value != 0; return CASV_OK;
    }
    if (!strcmp(key, "encoder_table")) {        // layer 1 of the search's per-step encoder from the per-character table (encoder.hip; same bits)
        if (value < 0 || value > 2) return fail(CASV_ERR_ARG, "encoder_table must be 0 (off), 1 (layer 1 where the pass qualifies) or 2 (and the upper layers' input terms ahead)");
        m->enc_table_opt = (int)value; return CASV_OK;
    }
    if (!strcmp(key, "beam_skip_last")) {       // debug switch: 0 = the search's last iteration launches its decoder step as every other (same results)
        if (value < 0 || value > 1) return fail(CASV_ERR_ARG, "beam_skip_last must be 0 or 1");
        m->beam_skip_last = value != 0; return CASV_OK;
    }
    if (!strcmp(key, "sample_cut_rows")) {      // test switch: at most this many rows per workgroup of sample_cut_kernel (same results)
        if (value < 0 || value > 4) return fail(CASV_ERR_ARG, "sample_cut_rows must be 0 (as many as fit) or 1 .. 4");
        m->sample_cut_rows_opt = (int)value; return CASV_OK;
    }
    if (!strcmp(key, "align_stamps")) {         // measurement aid: consensus_align_kernel adds up its waves' clocks in the fill and in the walk (same results)
        if (value < 0 || value > 1) return fail(CASV_ERR_ARG, "align_stamps must be 0 or 1");
        m->align_stamps = value != 0; return CASV_OK;
    }
    if (!strcmp(key, "vendor_gemm")) { m->vendor_gemm = value != 0; return CASV_OK; }
    if (!strcmp(key, "skinny") || !strcmp(key, "tile")) {   // process-wide: tile shape of the GEMM launches (results identical)
        if (value < -1 || value > 2) return fail(CASV_ERR_ARG, "tile must be -1 (by size), 0 (128x128), 1 (32x128) or 2 (64x128 where there is no split-K)");
        set_gemm_tile_mode((int)value); return CASV_OK;
    }
    if (!strcmp(key, "arithmetic")) {           // this handle's GEMM arithmetic (engine.h, arithmetic_of)
        if (value < -1 || value > 2) return fail(CASV_ERR_ARG, "arithmetic must be -1 (by entry point), 0 (fp32-input chain), 1 or 2 (bf16x3-split operands)");
        m->arith = (int)value; return CASV_OK;
    }
    if (!strcmp(key, "split_bf16")) {           // process-wide override of every handle's choice (tests, A/B measurements)
        if (value < -1 || value > 2) return fail(CASV_ERR_ARG, "split_bf16 must be -1 (no override), 0, 1 or 2");
        set_gemm_split_override((int)value); return CASV_OK;
    }
    return fail(CASV_ERR_ARG, "unknown option '%s'", key);
}

extern "C" int casv_synchronize(casv_model* m) {
    if (!m) return fail(CASV_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(m->device));
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}
