// The training session's state (train_state.h): built from the handle's Keras-layout weights by walking the Keras table, released
// as a whole; the session's entry points (begin, release, end, sync_weights) and the accessors that read or write ONE Keras tensor
// of it -- gradient, Adam's moments, step count.  Keras layouts exist only here, at set / get time: the step (train.hip) and the
// scoring calls (score.hip) work on the packed tensors.
#include "train_state.h"

namespace casv {

static int add_tensor(TrainState* ts, const std::string& name, const std::vector<float>& host, bool frozen) {
    ts->tens.emplace_back();
    TTensor& t = ts->tens.back();
    t.name = name; t.n = host.size(); t.frozen = frozen;
    const size_t bytes = host.size() * 4;
    if (t.w.ensure(bytes)) return -1;
    if (hipMemcpy(t.w.p, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return -1;
    if (ts->forward_only) return 0;       // (a scoring state: weights only)
    if (t.g.ensure(bytes) || t.m.ensure(bytes) || t.v.ensure(bytes)) return -1;
    (void)hipMemset(t.m.p, 0, bytes); (void)hipMemset(t.v.p, 0, bytes); (void)hipMemset(t.g.p, 0, bytes);
    return 0;
}

static bool is_frozen(const std::string& name, const std::string& csv) {
    size_t pos = 0;
    while (pos < csv.size()) {
        size_t e = csv.find(',', pos);
        if (e == std::string::npos) e = csv.size();
        const std::string p = csv.substr(pos, e - pos);
        if (!p.empty() && name.compare(0, p.size(), p) == 0) return true;
        pos = e + 1;
    }
    return false;
}

void release_state(casv_model* m, TrainState* ts) {
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->stream);
    if (ts->side) { (void)hipStreamSynchronize(ts->side); (void)hipStreamDestroy(ts->side); if (ts->ev_fork) (void)hipEventDestroy(ts->ev_fork); if (ts->ev_join) (void)hipEventDestroy(ts->ev_join); ts->side = nullptr; }
    delete ts;
}

void refresh_derived(casv_model* m, TrainState* ts) {
    const int W = m->W, V = m->V, Vp = m->Vp, C = m->C;
    for (auto& l : ts->layers) {
        launch_transpose(ts->W_(l.iwx), 4 * W, l.kx, l.kx, l.wxT.as<float>(), 4 * W, m->stream);
        launch_transpose(ts->W_(l.iwr), 4 * W, l.kr, l.kr, l.wrT.as<float>(), 4 * W, m->stream);
    }
    launch_transpose(ts->W_(ts->iE), V, W, W, ts->ETp.as<float>(), Vp, m->stream);
    launch_transpose(ts->W_(ts->iWaT), W, W, W, ts->WaN.as<float>(), W, m->stream);
    launch_transpose(ts->W_(ts->iUT), W, C, C, ts->UaN.as<float>(), W, m->stream);
    for (auto& b : ts->bridge) launch_transpose(ts->W_(b.ikt), W, W, W, b.kn.as<float>(), W, m->stream);
}

int build_state(casv_model* m, TrainState* ts, const std::string& fz) {
    const int W = m->W, D = m->D, C = m->C, Vp = m->Vp;
    ts->table = keras_table(W, m->V, C, D, m->cfg.deep_bidirectional_encoder != 0, m->cfg.bridge_dense != 0);
    int rc = 0;
    for (const KerasEntry& e : ts->table) {
        if (e.part[0] < (int)ts->tens.size()) continue;         // (an LSTM's R and b: packed with its K)
        std::vector<float> p[3];
        keras_pack(W, e, m->host, p);
        const bool frozen = !e.group.empty() && is_frozen(e.group + "_", fz);
        for (int j = 0; j < e.parts(); ++j) rc |= add_tensor(ts, e.packed_name(j), p[j], frozen);
        if (e.lstm()) {
            TLayer l;
            l.name = e.group; l.kx = e.kx; l.kr = e.kctx + W; l.encoder = e.encoder; l.dir = e.dir; l.reverse = e.dir == 1;
            l.iwx = e.part[0]; l.iwr = e.part[1]; l.ib = e.part[2];
            if (l.wxT.ensure((size_t)l.kx * 4 * W * 4) || l.wrT.ensure((size_t)l.kr * 4 * W * 4)) rc |= -1;
            ts->layers.push_back(std::move(l));
        } else if (!e.group.empty() && e.form == KerasEntry::TRANSPOSED) {      // a bridge's kernel; its bias is the next entry
            ts->bridge.emplace_back();
            ts->bridge.back().ikt = e.part[0];
            if (ts->bridge.back().kn.ensure((size_t)W * W * 4)) rc |= -1;
        } else if (!e.group.empty()) ts->bridge.back().ib = e.part[0];
    }
    if (rc) return fail(CASV_ERR_NOMEM, "could not allocate the training tensors");
    auto part = [&](const char* name) { return keras_find(ts->table, name)->part[0]; };
    ts->iE = part("E"); ts->iUT = part("att_U"); ts->iWaT = part("att_Wa"); ts->ibUW = part("att_bUW"); ts->iva = part("att_va"); ts->ibv = part("att_bv");
    if (ts->ETp.ensure((size_t)W * Vp * 4) || ts->WaN.ensure((size_t)W * W * 4) || ts->UaN.ensure((size_t)C * W * 4) ||
        ts->loss.ensure(16) || ts->normsq.ensure(16)) return fail(CASV_ERR_NOMEM, "out of memory");
    HIPCHK(hipMemset(ts->ETp.p, 0, (size_t)W * Vp * 4));
    ts->O.resize(D + 1); ts->DO.resize(D + 1); ts->XD.resize(D + 1);
    refresh_derived(m, ts);
    HIPCHK(hipStreamSynchronize(m->stream));
    return CASV_OK;
}

// Which buffer of a packed tensor: the master weights (0), the last gradients (1), Adam's m (2) / v (3).
static DevBuf& which_buf(TTensor& t, int which) { return which == 0 ? t.w : which == 1 ? t.g : which == 2 ? t.m : t.v; }

// Keras-layout values of ONE tensor from buffer `which`, into out[e.name] -- only the packed tensors that hold it are copied: an
// LSTM tensor comes with its layer's other two (K / R / b pack into Wx, Wr and the bias together), everything else alone.
static int fetch_keras(casv_model* m, TrainState* ts, int which, const KerasEntry& e, KerasView& out) {
    HIPCHK(hipStreamSynchronize(m->stream));
    std::vector<float> p[3];
    for (int j = 0; j < e.parts(); ++j) {
        TTensor& t = ts->tens[e.part[j]];
        p[j].resize(t.n);
        HIPCHK(hipMemcpy(p[j].data(), which_buf(t, which).p, t.n * 4, hipMemcpyDeviceToHost));
    }
    keras_unpack(m->W, e, p, out);
    return 0;
}

// ... and `values` (e.count() of them) into buffer `which`: an LSTM tensor is packed again with its layer's other two as the device holds them.
static int store_keras(casv_model* m, TrainState* ts, int which, const KerasEntry& e, const float* values) {
    KerasView view;
    if (e.lstm()) if (int rc = fetch_keras(m, ts, which, e, view)) return rc;
    view[e.name].assign(values, values + e.count());
    std::vector<float> p[3];
    keras_pack(m->W, e, view, p);
    for (int j = 0; j < e.parts(); ++j)
        HIPCHK(hipMemcpy(which_buf(ts->tens[e.part[j]], which).p, p[j].data(), p[j].size() * 4, hipMemcpyHostToDevice));
    return 0;
}

// The session's master weights in Keras layout, into the handle's host tensors.
static int weights_to_host(casv_model* m) {
    KerasView view;
    for (const KerasEntry& e : m->train->table)
        if (!view.count(e.name)) if (int rc = fetch_keras(m, m->train, 0, e, view)) return rc;
    for (auto& kv : view) m->host[kv.first] = std::move(kv.second);
    return 0;
}

// What the state accessors check, in this order: the session, `which`, the name, that the tensor is trained.
static int state_check(casv_model* m, const char* name, int which, const KerasEntry*& e) {
    if (!m || !name) return fail(CASV_ERR_ARG, "null argument");
    if (!m->train) return fail(CASV_ERR_STATE, "no training session");
    if (which != 0 && which != 1) return fail(CASV_ERR_ARG, "which must be 0 (Adam m) or 1 (Adam v)");
    e = keras_find(m->train->table, name);
    if (!e) return fail(CASV_ERR_ARG, "unknown tensor '%s'", name);
    if (m->train->tens[e->part[0]].frozen) return fail(CASV_ERR_STATE, "tensor '%s' is frozen: it has no optimizer state", name);
    return 0;
}

// One Keras tensor of buffer `which` into the caller's `out`.
static int get_keras(casv_model* m, int which, const KerasEntry& e, float* out, int64_t capacity) {
    HIPCHK(hipSetDevice(m->device));
    if ((size_t)capacity < e.count()) return fail(CASV_ERR_ARG, "buffer too small");
    KerasView view;
    if (int rc = fetch_keras(m, m->train, which, e, view)) return rc;
    memcpy(out, view[e.name].data(), e.count() * 4);
    return CASV_OK;
}

}  // namespace casv

int casv_train_release(casv_model* m) {
    if (!m || !m->train) return 0;
    release_state(m, m->train);
    m->train = nullptr;
    return 0;
}

extern "C" int casv_train_begin(casv_model* m, const casv_adam_params* ap, const char* frozen_csv) {
    if (!m || !ap) return fail(CASV_ERR_ARG, "null argument");
    if (m->W > 1024) return fail(CASV_ERR_ARG, "training supports width <= 1024");
    HIPCHK(hipSetDevice(m->device));
    for (auto& kv : m->expect)
        if (!m->host.count(kv.first)) return fail(CASV_ERR_STATE, "weight '%s' has not been set", kv.first.c_str());
    casv_train_release(m);
    (void)casv_score_release(m);
    TrainState* ts = new TrainState();
    m->train = ts;
    ts->ap = *ap;
    if (int rc = build_state(m, ts, frozen_csv ? frozen_csv : "")) { casv_train_release(m); return rc; }
    return CASV_OK;
}

extern "C" int casv_train_get_gradient(casv_model* m, const char* name, float* out, int64_t capacity) {
    if (!m || !name || !out) return fail(CASV_ERR_ARG, "null argument");
    if (!m->train) return fail(CASV_ERR_STATE, "no training session");
    const KerasEntry* e = keras_find(m->train->table, name);
    if (!e) return fail(CASV_ERR_ARG, "unknown tensor '%s'", name);
    return get_keras(m, 1, *e, out, capacity);
}

// ---- optimizer state (resumable training) ----
extern "C" int casv_train_get_state(casv_model* m, const char* name, int32_t which, float* out, int64_t capacity) {
    const KerasEntry* e = nullptr;
    if (int rc = state_check(m, name, which, e)) return rc;
    if (!out) return fail(CASV_ERR_ARG, "null argument");
    return get_keras(m, 2 + which, *e, out, capacity);
}

extern "C" int casv_train_set_state(casv_model* m, const char* name, int32_t which, const float* data, int64_t count) {
    const KerasEntry* e = nullptr;
    if (int rc = state_check(m, name, which, e)) return rc;
    if (!data) return fail(CASV_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(m->device));
    if ((size_t)count != e->count()) return fail(CASV_ERR_ARG, "tensor '%s' has %zu values, got %lld", name, e->count(), (long long)count);
    return store_keras(m, m->train, 2 + which, *e, data);
}

extern "C" int casv_train_get_step(casv_model* m, int64_t* step) {
    if (!m || !step) return fail(CASV_ERR_ARG, "null argument");
    if (!m->train) return fail(CASV_ERR_STATE, "no training session");
    *step = m->train->step;
    return CASV_OK;
}

extern "C" int casv_train_set_step(casv_model* m, int64_t step) {
    if (!m) return fail(CASV_ERR_ARG, "null argument");
    if (!m->train) return fail(CASV_ERR_STATE, "no training session");
    if (step < 0) return fail(CASV_ERR_ARG, "step must be >= 0");
    m->train->step = (long)step;
    return CASV_OK;
}

// Copy the current master weights into the handle's Keras-layout tensors without ending the session
// (ModelCheckpoint / EarlyStopping(restore_best_weights), seq2seq.py:619-622).
extern "C" int casv_train_sync_weights(casv_model* m) {
    if (!m) return fail(CASV_ERR_ARG, "null argument");
    if (!m->train) return fail(CASV_ERR_STATE, "no training session");
    HIPCHK(hipSetDevice(m->device));
    return weights_to_host(m);
}

// Bring the trained weights back into the handle (Keras layout) and repack them for inference
// (the reference's _resync_decoder after training, seq2seq.py:645).
extern "C" int casv_train_end(casv_model* m) {
    if (!m) return fail(CASV_ERR_ARG, "null argument");
    if (!m->train) return fail(CASV_ERR_STATE, "no training session");
    HIPCHK(hipSetDevice(m->device));
    if (int rc = weights_to_host(m)) return rc;
    casv_train_release(m);
    return casv_commit_weights(m);
}
