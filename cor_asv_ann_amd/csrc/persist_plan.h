// The plans of the decode path's persistent launches -- the greedy decoder (persist.hip: persist_decode_kernel) and the encoder in
// its two arithmetics (persist.hip: persist_encode_kernel; persist_split.hip: persist_split_encode_kernel) -- as pure functions of
// the shape, the device's CU count, the workgroups per CU the runtime admits for the kernel (persist_host.h asks for it, the host
// hands it in), the option "persistent" and the arithmetic.  Nothing here knows the device or the environment: a stand-alone
// driver (tests/persist_plan_driver.cpp) plans the case table of tests/persist_form_cases.py on the CPU.
// decode.hip and encoder.hip launch what these functions return; the kernels read the role sizes and the grid from their arguments.
#pragma once
#include <algorithm>
#include <cstddef>

namespace casv {

constexpr int PERSIST_MIN_CUS = 64;                 // below: no persistent launch of the decode path
constexpr int PERSIST_MAX_DEPTH = 8;                // PersistArgs::layer[8], PersistEncArgs::ln[7]
constexpr size_t PERSIST_LDS_LIMIT = 150 * 1024;    // staged rows of persist.hip's two kernels: no launch form above
constexpr int PERSIST_MAX_ROWS_FORCED = 4096;       // "persistent" = 1: up to this many lines
constexpr int PERSIST_MAX_ROWS_DEFAULT = 512;       // "persistent" = -1, fp32-input chain
constexpr int PERSIST_MAX_OWN_DEFAULT = 2;          // ... and at most this many tiles per workgroup and layer (phase)
constexpr int PERSIST_ENC_MAX_TILES = 8;            // persist.hip: PENC_MAXT
constexpr int PERSIST_SPLIT_MAX_TILES = 4;          // persist_split.hip: PS_MAXT
// Rows up to which the split-arithmetic persistent encoder is the default form of a pass (option "persistent" = -1): the largest
// batch of profiles/split_persist_encoder_timing.json at which its median lies below the per-step launches' by more than the
// spread of the repetitions.
constexpr int PERSIST_SPLIT_DEFAULT_ROWS = 256;

inline size_t persist_counter_bytes_of(size_t counters) { return (counters * 32 + 32) * sizeof(unsigned); }    // persist_host.h: persist_counters_bytes

// ---- the greedy decoder ----
struct PersistDecShape { int D, W, Vp, C; };        // depth, width, padded vocabulary, attended width
// widest contraction of any task of the launch: layer 1 reads [p | (ctx) | h], the layers above [x | (ctx) | h], the top one the context
inline int persist_dec_kmax(const PersistDecShape& s) {
    int kmax = s.W;
    for (int n = 1; n <= s.D; ++n) kmax = std::max(kmax, (n == 1 ? s.Vp : s.W) + (n == s.D ? s.C : 0) + s.W);
    return kmax;
}
inline int persist_dec_lda(const PersistDecShape& s) { return persist_dec_kmax(s) + 4; }
inline size_t persist_dec_lds_bytes(const PersistDecShape& s) { return (size_t)16 * persist_dec_lda(s) * sizeof(float); }

struct PersistDecPlan {
    enum Reason { OK, OFF, SPLIT_ARITHMETIC, CUS, DEPTH, LDS, NOT_WORTH } reason = OFF;    // why the decode is not persistent (OK: it is; NOT_WORTH: the size rule)
    bool applies = false;
    int kmax = 0, lda = 0; size_t lds_bytes = 0;
    int per_cu = 0;                                 // workgroups per CU the plan counted on
    int g_lstm = 0, g_att = 0, g_plain = 0;         // workgroups per role
    size_t counter_bytes = 0;
};
// The role sizes of a launch over R rows: every workgroup must be resident at once (they wait for each other), the roles share the
// wgslots = CUs x per_cu slots 4 : 1 : 2 (tiles, attention, plain).
inline void persist_dec_roles(const PersistDecShape& s, int R, int ncu, int per_cu, PersistDecPlan& p) {
    const int nrb = (R + 15) / 16, nug = s.W / 16;
    const int nq4 = (s.W / 16 + 3) / 4, nl4 = (s.Vp / 16 + 3) / 4;
    const int wgslots = ncu * per_cu;
    p.g_lstm = std::min(nrb * nug, wgslots * 4 / 8);
    p.g_plain = std::min(nrb * (nq4 + nl4), std::max(wgslots * 2 / 8, 4));
    // (attention: one workgroup per four rows where the slots the other roles leave allow it -- a wave then keeps its row, persist.hip)
    p.g_att = std::min(nrb * 4, std::max(std::max(wgslots / 8, 4), wgslots - p.g_lstm - p.g_plain));
}
// Whether casv_decode_greedy over B lines runs as the persistent launch, and that launch.  per_cu: the runtime's figure for
// persist_decode_kernel at persist_dec_lds_bytes(s) (0 where those exceed PERSIST_LDS_LIMIT: the host does not ask then).
// persistent: the option (0 never, 1 always, anything else by size); arithmetic: of the entry point (the kernel is an fp32-input one).
inline PersistDecPlan plan_persist_decode(const PersistDecShape& s, int B, int ncu, int per_cu, int persistent, int arithmetic) {
    PersistDecPlan p;
    p.kmax = persist_dec_kmax(s); p.lda = p.kmax + 4; p.lds_bytes = persist_dec_lds_bytes(s);
    p.per_cu = p.lds_bytes > PERSIST_LDS_LIMIT ? 0 : per_cu;
    auto no = [&](PersistDecPlan::Reason r) { p.reason = r; return p; };
    if (persistent == 0) return no(PersistDecPlan::OFF);
    if (arithmetic) return no(PersistDecPlan::SPLIT_ARITHMETIC);    // (not mixed with split launches)
    if (ncu < PERSIST_MIN_CUS) return no(PersistDecPlan::CUS);
    if (s.D > PERSIST_MAX_DEPTH) return no(PersistDecPlan::DEPTH);
    if (p.per_cu < 1) return no(PersistDecPlan::LDS);                // the staged rows must fit the LDS
    persist_dec_roles(s, B, ncu, p.per_cu, p);
    p.counter_bytes = persist_counter_bytes_of((size_t)((B + 15) / 16) * (s.D + 3));
    if (persistent == 1) {
        if (B > PERSIST_MAX_ROWS_FORCED) return no(PersistDecPlan::NOT_WORTH);
    } else {
        // by size: the persistent kernel wins while a workgroup owns at most two tiles per layer (measured: depth 2, width 512: 64
        // lines 9.3 vs 20.9 ms, 256 lines 32.5 vs 21.4 ms; depth 2, width 256: 512 lines 11.4 vs 14.7 ms)
        if (B > PERSIST_MAX_ROWS_DEFAULT) return no(PersistDecPlan::NOT_WORTH);
        const int g_lstm = std::max(1, ncu * p.per_cu * 4 / 8), ntile = ((B + 15) / 16) * (s.W / 16);
        if ((ntile + g_lstm - 1) / g_lstm > PERSIST_MAX_OWN_DEFAULT) return no(PersistDecPlan::NOT_WORTH);
    }
    p.applies = true;
    return no(PersistDecPlan::OK);
}

// ---- the encoder ----
struct PersistEncShape { int D, W; bool residual, deep; };        // depth, width, residual_connections, deep_bidirectional_encoder
// staged rows of the chain kernel: [x | h] of layer 1 (2W), [fw | bw | h] of layer 2 (3W)
inline int persist_enc_lda(const PersistEncShape& s) { return (s.D >= 2 ? 3 * s.W : 2 * s.W) + 4; }
inline size_t persist_enc_lds_bytes(const PersistEncShape& s) { return (size_t)16 * persist_enc_lda(s) * sizeof(float); }

struct PersistEncPlan {
    enum Form { NONE, CHAIN, SPLIT } form = NONE;
    enum Reason { OK, OFF, CUS, DEPTH, TOPOLOGY, LDS, OWN, NOT_WORTH } reason = OFF;     // why there is no persistent form (OK: there is; OWN: more tiles per workgroup than the kernel holds; NOT_WORTH: the size rule)
    int grid = 0;                   // workgroups, all resident at once
    int per_cu = 0;                 // workgroups per CU the plan counted on
    int own1 = 0, ownn = 0;         // tiles per workgroup in the launch's two phases (layer 1's two directions; the layers above)
    size_t counter_bytes = 0;       // their hand-off counters
};
// Whether a pass over B lines has a persistent form, and that form's launch -- planned once, for the decision and the launch alike.
// split: the pass runs in the split arithmetic (tiles of 32 x 32, a fixed LDS size); per_cu: the runtime's figure for the form's
// kernel (chain: at persist_enc_lds_bytes(s), 0 where those exceed PERSIST_LDS_LIMIT).
inline PersistEncPlan plan_persist_encode(const PersistEncShape& s, int B, int ncu, int per_cu, int persistent, bool split) {
    PersistEncPlan p;
    auto no = [&](PersistEncPlan::Reason r) { p.form = PersistEncPlan::NONE; p.reason = r; return p; };
    if (persistent == 0) return no(PersistEncPlan::OFF);
    if (ncu < PERSIST_MIN_CUS) return no(PersistEncPlan::CUS);
    if (s.D > PERSIST_MAX_DEPTH) return no(PersistEncPlan::DEPTH);
    if (s.residual && s.D >= 3) return no(PersistEncPlan::TOPOLOGY);   // (the layers' sums of seq2seq.py:284-291 have no persistent form)
    if (s.deep && s.D >= 2) return no(PersistEncPlan::TOPOLOGY);
    const int W = s.W, D = s.D;
    const int side = split ? 32 : 16;
    p.per_cu = !split && persist_enc_lds_bytes(s) > PERSIST_LDS_LIMIT ? 0 : per_cu;      // 0: the staged rows do not fit the LDS
    if (p.per_cu < 1) return no(PersistEncPlan::LDS);
    const int ntile = ((B + side - 1) / side) * (W / side);
    p.grid = std::min(std::max(2, D - 1) * ntile, p.per_cu * ncu);
    p.own1 = (2 * ntile + p.grid - 1) / p.grid; p.ownn = ((D - 1) * ntile + p.grid - 1) / p.grid;
    p.counter_bytes = persist_counter_bytes_of((size_t)((B + side - 1) / side) * (D + 1));
    const int maxt = split ? PERSIST_SPLIT_MAX_TILES : PERSIST_ENC_MAX_TILES;
    if (p.own1 > maxt || p.ownn > maxt) return no(PersistEncPlan::OWN);
    const bool pays = persistent == 1 ? B <= PERSIST_MAX_ROWS_FORCED
                    : split ? B <= PERSIST_SPLIT_DEFAULT_ROWS
                            : B <= PERSIST_MAX_ROWS_DEFAULT && p.own1 <= PERSIST_MAX_OWN_DEFAULT && p.ownn <= PERSIST_MAX_OWN_DEFAULT;
    if (!pays) return no(PersistEncPlan::NOT_WORTH);
    p.form = split ? PersistEncPlan::SPLIT : PersistEncPlan::CHAIN;
    p.reason = PersistEncPlan::OK;
    return p;
}

}  // namespace casv
