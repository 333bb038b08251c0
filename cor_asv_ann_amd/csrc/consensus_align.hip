// Host side of casv_consensus_align, casv_consensus_align_costed and casv_consensus_vote (include/cor_asv_ann_hip.h): the checks, the
// handle's buffers, the rounds of consensus_align_kernel under the direction-word budget, the layout and the vote launches of
// consensus_kernels.hip on the handle's stream.  The pair owns the al_* buffers of the handle: no buffer of casv_consensus or of an
// encode, decode, score or train session is read or written.
#include "engine.h"
#include <cmath>

// Both align entry points: costs == nullptr is the plain call (key is not looked at), else the costed one
static int align_call(casv_model* m, int32_t B, int32_t N, int32_t L, const int32_t* sym, const int32_t* key, const int32_t* len,
                      const int32_t* pivot, const EditCosts* costs, int32_t* out_where, int32_t* out_ncol) {
    if (!m || !len || !pivot || !out_ncol || (L > 0 && (!sym || !out_where))) return fail(CASV_ERR_ARG, "null argument");
    if (costs) if (const char* why = edit_costs_refused(*costs)) return fail(CASV_ERR_ARG, "costs {%d, %d, %d, %d}: %s", costs->gap, costs->sub, costs->near, costs->unit, why);
    if (B < 1) return fail(CASV_ERR_ARG, "B=%d: need at least one source", B);
    if (N < 1 || N > CONSENSUS_MAX_N) return fail(CASV_ERR_ARG, "N=%d out of range 1..%d", N, CONSENSUS_MAX_N);
    if (L < 0 || L > CONSENSUS_ALIGN_MAX_L) return fail(CASV_ERR_ARG, "L=%d out of range 0..%d", L, CONSENSUS_ALIGN_MAX_L);
    const size_t rows = (size_t)B * N;
    int max_len = 0, max_pivot = 0;
    for (size_t r = 0; r < rows; ++r) {
        if (len[r] < -1 || len[r] > L) return fail(CASV_ERR_ARG, "len[%zu]=%d outside -1..%d", r, len[r], L);
        max_len = std::max(max_len, len[r]);
    }
    for (int b = 0; b < B; ++b) {
        if (pivot[b] < -1 || pivot[b] >= N) return fail(CASV_ERR_ARG, "pivot[%d]=%d outside -1..%d", b, pivot[b], N - 1);
        if (pivot[b] < 0) continue;
        const int lp = len[(size_t)b * N + pivot[b]];
        if (lp < 0) return fail(CASV_ERR_ARG, "pivot[%d]=%d names a padding candidate", b, pivot[b]);
        max_pivot = std::max(max_pivot, lp);
    }
    HIPCHK(hipSetDevice(m->device));
    // one round's sources: as many as the budget holds direction words for, at least one
    const size_t pair = consensus_align_pair_bytes(max_pivot, max_len), source = std::max(pair * N, (size_t)1);
    const size_t budget = m->align_budget ? m->align_budget : CONSENSUS_ALIGN_BUDGET;
    const int per_round = (int)std::max((size_t)1, std::min((size_t)B, budget / source));
    const size_t nsym = rows * (size_t)L, stride = (size_t)max_len + 1;
    m->al_valid = false;                         // (from here on the buffers no longer hold the call before)
    if (int rc = m->al_sym.ensure(std::max(nsym, (size_t)1) * 4)) return rc;
    if (int rc = m->al_where.ensure(std::max(nsym, (size_t)1) * 4)) return rc;
    const bool keyed = costs && key && nsym;
    if (keyed) if (int rc = m->al_key.ensure(nsym * 4)) return rc;
    if (int rc = m->al_len.ensure(rows * 4)) return rc;
    if (int rc = m->al_pivot.ensure((size_t)B * 4)) return rc;
    if (int rc = m->al_ncol.ensure((size_t)B * 4)) return rc;
    if (int rc = m->al_ins.ensure((size_t)B * stride * 4)) return rc;
    if (int rc = m->al_start.ensure((size_t)B * stride * 4)) return rc;
    if (int rc = m->al_dir.ensure(source * per_round)) return rc;
    if (nsym) HIPCHK(hipMemcpyAsync(m->al_sym.p, sym, nsym * 4, hipMemcpyHostToDevice, m->stream));
    if (keyed) HIPCHK(hipMemcpyAsync(m->al_key.p, key, nsym * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->al_len.p, len, rows * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->al_pivot.p, pivot, (size_t)B * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemsetAsync(m->al_ins.p, 0, (size_t)B * stride * 4, m->stream));
    if (m->align_stamps) {
        if (int rc = m->al_stamps.ensure(16)) return rc;
        HIPCHK(hipMemsetAsync(m->al_stamps.p, 0, 16, m->stream));
    }
    AlignArgs a{};
    a.sym = m->al_sym.as<int>(); a.len = m->al_len.as<int>(); a.pivot = m->al_pivot.as<int>();
    a.where = m->al_where.as<int>(); a.ins = m->al_ins.as<int>(); a.start = m->al_start.as<int>(); a.ncol = m->al_ncol.as<int>();
    a.dir = m->al_dir.as<uint2>(); a.stamps = m->align_stamps ? m->al_stamps.as<unsigned long long>() : nullptr;
    a.B = B; a.N = N; a.L = L; a.stride = (int)stride; a.rows = max_pivot; a.wpr = consensus_align_wpr(max_len);
    a.key = !costs ? nullptr : keyed ? m->al_key.as<int>() : a.sym;      // (no keys: the symbols as keys -- equal only where those are)
    a.costs = costs ? *costs : EditCosts{1, 1, 1, 1};
    hipEvent_t ev{};
    m->prof_begin(PC_CONSENSUS, 0.0, 8.0 * (double)nsym + 2.0 * (double)pair * (double)rows, ev);
    m->stat_align_rounds = 0;
    for (int b0 = 0; b0 < B; b0 += per_round) {
        a.b0 = b0; a.b1 = std::min(B, b0 + per_round);
        launch_consensus_align(a, max_len, m->stream);
        ++m->stat_align_rounds;
    }
    launch_consensus_layout(a, m->stream);
    m->prof_end(PC_CONSENSUS, ev);
    HIPCHK(hipGetLastError());
    if (nsym) HIPCHK(hipMemcpyAsync(out_where, a.where, nsym * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_ncol, a.ncol, (size_t)B * 4, hipMemcpyDeviceToHost, m->stream));
    m->stat_align_ticks[0] = m->stat_align_ticks[1] = 0;
    if (a.stamps) HIPCHK(hipMemcpyAsync(m->stat_align_ticks, a.stamps, 16, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->prof.on) m->prof.collect();
    m->al_B = B; m->al_N = N; m->al_L = L; m->al_stride = (int)stride;
    m->al_max_ncol = 0;
    for (int b = 0; b < B; ++b) m->al_max_ncol = std::max(m->al_max_ncol, out_ncol[b]);
    m->al_valid = true;
    return CASV_OK;
}

extern "C" int casv_consensus_align(casv_model* m, int32_t B, int32_t N, int32_t L, const int32_t* sym, const int32_t* len,
                                    const int32_t* pivot, int32_t* out_where, int32_t* out_ncol) {
    return align_call(m, B, N, L, sym, nullptr, len, pivot, nullptr, out_where, out_ncol);
}

extern "C" int casv_consensus_align_costed(casv_model* m, int32_t B, int32_t N, int32_t L, const int32_t* sym, const int32_t* key,
                                           const int32_t* len, const int32_t* pivot, const casv_edit_costs* costs, int32_t* out_where,
                                           int32_t* out_ncol) {
    if (!costs) return fail(CASV_ERR_ARG, "null argument");
    const EditCosts ec{costs->gap, costs->sub, costs->near, costs->unit};
    return align_call(m, B, N, L, sym, key, len, pivot, &ec, out_where, out_ncol);
}

extern "C" int casv_consensus_vote(casv_model* m, int32_t C, const double* weight, int32_t* out_src, double* out_mass, int32_t* out_best) {
    if (!m) return fail(CASV_ERR_ARG, "null argument");
    if (!m->al_valid) return fail(CASV_ERR_STATE, "casv_consensus_vote: no casv_consensus_align to read");
    if (!out_src || !out_mass || !out_best) return fail(CASV_ERR_ARG, "null argument");
    if (C < 1 || C < m->al_max_ncol) return fail(CASV_ERR_ARG, "C=%d: need at least max(1, %d columns)", C, m->al_max_ncol);
    const int B = m->al_B, N = m->al_N;
    const size_t rows = (size_t)B * N, cells = rows * (size_t)C;
    if (weight)
        for (size_t r = 0; r < rows; ++r)
            if (!(weight[r] >= 0.0) || !std::isfinite(weight[r])) return fail(CASV_ERR_ARG, "weight[%zu]=%g: must be finite and not negative", r, weight[r]);
    HIPCHK(hipSetDevice(m->device));
    if (weight) if (int rc = m->al_weight.ensure(rows * 8)) return rc;
    if (int rc = m->al_src.ensure(cells * 4)) return rc;
    if (int rc = m->al_mass.ensure(cells * 8)) return rc;
    if (int rc = m->al_best.ensure((size_t)B * C * 4)) return rc;
    if (weight) HIPCHK(hipMemcpyAsync(m->al_weight.p, weight, rows * 8, hipMemcpyHostToDevice, m->stream));
    VoteArgs a{};
    a.sym = m->al_sym.as<int>(); a.len = m->al_len.as<int>(); a.pivot = m->al_pivot.as<int>(); a.where = m->al_where.as<int>();
    a.ins = m->al_ins.as<int>(); a.start = m->al_start.as<int>(); a.ncol = m->al_ncol.as<int>();
    a.weight = weight ? m->al_weight.as<double>() : nullptr;
    a.src = m->al_src.as<int>(); a.mass = m->al_mass.as<double>(); a.best = m->al_best.as<int>();
    a.B = B; a.N = N; a.L = m->al_L; a.stride = m->al_stride; a.C = C;
    hipEvent_t ev{};
    m->prof_begin(PC_CONSENSUS, 0.0, 16.0 * (double)cells, ev);
    launch_consensus_vote(a, m->stream);
    m->prof_end(PC_CONSENSUS, ev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_src, a.src, cells * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_mass, a.mass, cells * 8, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_best, a.best, (size_t)B * C * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->prof.on) m->prof.collect();
    return CASV_OK;
}

extern "C" int casv_debug_set_align_budget(casv_model* m, int64_t bytes) {
    if (!m || bytes < 0) return fail(CASV_ERR_ARG, "casv_debug_set_align_budget: null handle or negative budget");
    m->align_budget = (size_t)bytes;
    return CASV_OK;
}
