// Host side of casv_consensus and casv_consensus_costed (include/cor_asv_ann_hip.h): the checks, the handle's scratch, the two launches
// of consensus_kernels.hip on the handle's stream.  The call touches no buffer of an encode, decode, score or train session.
#include "engine.h"
#include <cmath>

// Both entry points: costs == nullptr is the plain call (key is not looked at), else the costed one
static int consensus_call(casv_model* m, int32_t B, int32_t N, int32_t L, int32_t mode, const int32_t* sym, const int32_t* key, const int32_t* len,
                          const double* weight, const EditCosts* costs, int32_t* out_dist, double* out_risk, int32_t* out_pick) {
    if (!m || !len || !out_risk || !out_pick || (L > 0 && !sym)) return fail(CASV_ERR_ARG, "null argument");
    const int max_L = costs ? CONSENSUS_COSTED_MAX_L : CONSENSUS_MAX_L;
    if (costs) if (const char* why = edit_costs_refused(*costs)) return fail(CASV_ERR_ARG, "costs {%d, %d, %d, %d}: %s", costs->gap, costs->sub, costs->near, costs->unit, why);
    if (B < 1) return fail(CASV_ERR_ARG, "B=%d: need at least one source", B);
    if (N < 1 || N > CONSENSUS_MAX_N) return fail(CASV_ERR_ARG, "N=%d out of range 1..%d", N, CONSENSUS_MAX_N);
    if (L < 0 || L > max_L) return fail(CASV_ERR_ARG, "L=%d out of range 0..%d", L, max_L);
    if (mode < 0 || mode > 1) return fail(CASV_ERR_ARG, "mode=%d out of range 0..1", mode);
    const size_t rows = (size_t)B * N;
    int max_len = 0;
    for (size_t r = 0; r < rows; ++r) {
        if (len[r] < -1 || len[r] > L) return fail(CASV_ERR_ARG, "len[%zu]=%d outside -1..%d", r, len[r], L);
        max_len = std::max(max_len, len[r]);
    }
    if (weight)
        for (size_t r = 0; r < rows; ++r)
            if (!(weight[r] >= 0.0) || !std::isfinite(weight[r])) return fail(CASV_ERR_ARG, "weight[%zu]=%g: must be finite and not negative", r, weight[r]);
    HIPCHK(hipSetDevice(m->device));
    if (!consensus_ready()) return fail(CASV_ERR_HIP, "the runtime refused consensus_dist_kernel's %d bytes of dynamic LDS", consensus_lds_bytes(CONSENSUS_MAX_L));
    const size_t nsym = rows * (size_t)L;
    if (int rc = m->cs_sym.ensure(std::max(nsym, (size_t)1) * 4)) return rc;
    const bool keyed = costs && key && nsym;
    if (keyed) if (int rc = m->cs_key.ensure(nsym * 4)) return rc;
    if (int rc = m->cs_len.ensure(rows * 4)) return rc;
    if (weight) if (int rc = m->cs_weight.ensure(rows * 8)) return rc;
    if (int rc = m->cs_dist.ensure(rows * N * 4)) return rc;
    if (int rc = m->cs_risk.ensure(rows * 8)) return rc;
    if (int rc = m->cs_pick.ensure((size_t)B * 4)) return rc;
    if (nsym) HIPCHK(hipMemcpyAsync(m->cs_sym.p, sym, nsym * 4, hipMemcpyHostToDevice, m->stream));
    if (keyed) HIPCHK(hipMemcpyAsync(m->cs_key.p, key, nsym * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(m->cs_len.p, len, rows * 4, hipMemcpyHostToDevice, m->stream));
    if (weight) HIPCHK(hipMemcpyAsync(m->cs_weight.p, weight, rows * 8, hipMemcpyHostToDevice, m->stream));
    ConsensusArgs a{};
    a.sym = m->cs_sym.as<int>(); a.len = m->cs_len.as<int>(); a.weight = weight ? m->cs_weight.as<double>() : nullptr;
    a.dist = m->cs_dist.as<int>(); a.risk = m->cs_risk.as<double>(); a.pick = m->cs_pick.as<int>();
    a.B = B; a.N = N; a.L = L; a.mode = mode;
    a.key = !costs ? nullptr : keyed ? m->cs_key.as<int>() : a.sym;      // (no keys: the symbols as keys -- equal only where those are)
    a.costs = costs ? *costs : EditCosts{1, 1, 1, 1};
    hipEvent_t ev{};
    m->prof_begin(PC_CONSENSUS, 0.0, (keyed ? 8.0 : 4.0) * (double)nsym + 8.0 * (double)rows * N, ev);
    launch_consensus_dist(a, max_len, m->stream);
    launch_consensus_risk(a, m->stream);
    m->prof_end(PC_CONSENSUS, ev);
    HIPCHK(hipGetLastError());
    if (out_dist) HIPCHK(hipMemcpyAsync(out_dist, a.dist, rows * N * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_risk, a.risk, rows * 8, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(out_pick, a.pick, (size_t)B * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->prof.on) m->prof.collect();
    return CASV_OK;
}

extern "C" int casv_consensus(casv_model* m, int32_t B, int32_t N, int32_t L, int32_t mode, const int32_t* sym, const int32_t* len,
                              const double* weight, int32_t* out_dist, double* out_risk, int32_t* out_pick) {
    return consensus_call(m, B, N, L, mode, sym, nullptr, len, weight, nullptr, out_dist, out_risk, out_pick);
}

extern "C" int casv_consensus_costed(casv_model* m, int32_t B, int32_t N, int32_t L, int32_t mode, const int32_t* sym, const int32_t* key,
                                     const int32_t* len, const double* weight, const casv_edit_costs* costs, int32_t* out_dist,
                                     double* out_risk, int32_t* out_pick) {
    if (!costs) return fail(CASV_ERR_ARG, "null argument");
    const EditCosts ec{costs->gap, costs->sub, costs->near, costs->unit};
    return consensus_call(m, B, N, L, mode, sym, key, len, weight, &ec, out_dist, out_risk, out_pick);
}
