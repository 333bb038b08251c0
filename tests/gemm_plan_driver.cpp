// Stand-alone driver of the GEMM launch planner (cor_asv_ann_amd/csrc/gemm_plan.h) for tests/test_gemm_plan.py: reads cases on
// stdin, one per line, and prints what each becomes -- one record per launch and clear -- on stdout.  Host code only.
//
//   G <name> key=value ... [; key=value ...]...     a forward batch: context / switch / epilogue keys, then one group per job
//   T <name> key=value ...                          one weight-gradient contraction
//
// Pointers are made up (a job's operands lie 4 GiB apart), so that a record shows which ones a cut has moved and by how much.
#include "../cor_asv_ann_amd/csrc/gemm_plan.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

using namespace casv;

// ---- cases ----
typedef std::map<std::string, long long> Keys;
static long long key(const Keys& k, const char* name, long long otherwise) { auto it = k.find(name); return it == k.end() ? otherwise : it->second; }
// (segs=, koffs=, lds=: comma-separated lists, one entry per K segment; koffs / lds default to ascending offsets and ld = width)
static Keys parse_keys(const std::string& text, std::vector<int>* segs, std::vector<int>* koffs = nullptr, std::vector<int>* lds = nullptr) {
    Keys k;
    std::istringstream in(text);
    std::string tok;
    while (in >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) { fprintf(stderr, "bad token %s\n", tok.c_str()); exit(2); }
        const std::string name = tok.substr(0, eq), val = tok.substr(eq + 1);
        std::vector<int>* list = name == "segs" ? segs : name == "koffs" ? koffs : name == "lds" ? lds : nullptr;
        if (list) {
            std::istringstream vs(val);
            std::string w;
            while (std::getline(vs, w, ',')) list->push_back(atoi(w.c_str()));
        } else k[name] = atoll(val.c_str());
    }
    return k;
}
template <class T> static T* fake(int job, int slot) { return reinterpret_cast<T*>(((unsigned long long)(job + 1) << 40) + ((unsigned long long)slot << 32)); }
static GemmArgs make_job(int epi, int j, const std::string& text) {
    std::vector<int> segs, koffs, lds;
    const Keys k = parse_keys(text, &segs, &koffs, &lds);
    GemmArgs g{};
    g.M = (int)key(k, "M", 0); g.N = (int)key(k, "N", 0);
    if (segs.empty()) segs.push_back((int)key(k, "K", 0));
    g.nseg = (int)segs.size();
    int koff = (int)key(k, "koff0", 0);
    for (int i = 0; i < g.nseg; ++i) {
        Seg& s = g.a[i];
        s.base = fake<const float>(j, 1 + i);
        if (key(k, "rows", 0) >> i & 1) s.rows = fake<const int>(j, 8 + i);
        if (key(k, "first", 0) >> i & 1) s.first_base = fake<const float>(j, 12 + i);
        s.skip_first = key(k, "skip", 0) >> i & 1;
        s.width = segs[i]; s.ld = i < (int)lds.size() ? lds[i] : (int)key(k, "ld", segs[i]); s.koff = i < (int)koffs.size() ? koffs[i] : koff;
        koff = s.koff + segs[i];
    }
    if (!koffs.empty()) { koff = 0; for (int i = 0; i < g.nseg; ++i) koff = std::max(koff, g.a[i].koff + g.a[i].width); }
    g.Ktot = (int)key(k, "Ktot", koff);
    g.Bt = fake<const float>(j, 22); g.bias = fake<const float>(j, 23);
    const bool lstm = epi == EPI_LSTM && !key(k, "epiplain", 0);
    g.out.base = fake<float>(j, 16); g.out.ld = (int)key(k, "outld", lstm ? g.N / 4 : g.N);
    g.out.slot_stride = key(k, "slot", 0); g.out.step_mul = 1;
    if (key(k, "cell", lstm)) {
        g.c_in.base = fake<const float>(j, 4); g.c_in.ld = g.N / 4; g.c_in.width = g.N / 4;
        if (key(k, "crows", 0)) g.c_in.rows = fake<const int>(j, 5);
        g.c_out.base = fake<float>(j, 17); g.c_out.ld = g.N / 4;
    }
    if (key(k, "zinit", 0)) { g.zinit.base = fake<float>(j, 18); g.zinit.ld = g.N; }
    if (key(k, "gates", 0)) { g.gates_out.base = fake<float>(j, 19); g.gates_out.ld = g.N; }
    if (key(k, "out2", 0)) { g.out2.base = fake<float>(j, 20); g.out2.ld = g.N / 4; }
    if (key(k, "nact", 0)) { g.nact = fake<const int>(j, 21); g.nact_group = (int)key(k, "nact", 0); }
    if (key(k, "stepptr", 0)) g.step_ptr = fake<const int>(j, 24);
    g.step_imm = (int)key(k, "step", 0);
    g.epi_plain = (int)key(k, "epiplain", 0); g.accumulate = (int)key(k, "acc", 0); g.out_zeroed = (int)key(k, "zeroed", 0);
    g.kgroups = (int)key(k, "kgroups", 0); g.b_static = (int)key(k, "bstatic", 0); g.ksplit = (int)key(k, "ksplit", 0);
    return g;
}
static GemmContext make_context(const Keys& k) { return GemmContext{(int)key(k, "ncu", 256), (int)key(k, "arith", 0), (int)key(k, "ordered", 0)}; }
static GemmSwitches make_switches(const Keys& k) {
    GemmSwitches s;
    s.tile_mode = (int)key(k, "tile", -1); s.tail_cut = key(k, "tail_cut", 1); s.split_tail_cut = key(k, "split_tail_cut", 1);
    s.tn_split = key(k, "tn_split", 1); s.split_images = key(k, "images", 1); s.lds_pad = (int)key(k, "lds_pad", 0);
    return s;
}
static TnArgs make_tn(const Keys& k) {
    TnArgs t{};
    t.M = (int)key(k, "M", 0); t.Mstore = (int)key(k, "Mstore", t.M); t.N = (int)key(k, "N", 0); t.K = (int)key(k, "K", 0);
    t.A = fake<const float>(0, 1); t.lda = t.M; t.B = fake<const float>(0, 2); t.ldb = t.N; t.C = fake<float>(0, 3); t.ldc = key(k, "ldc", t.N);
    t.accumulate = (int)key(k, "acc", 0); t.out_zeroed = (int)key(k, "zeroed", 0);
    return t;
}

// ---- records ----
static unsigned long long rec_p(const void* p) { return (unsigned long long)(size_t)p; }
static void rec_job(const GemmArgs& g) {
    printf(" | M=%d N=%d ks=%d xcd=%d ep=%d", g.M, g.N, g.ksplit, g.xcd_rows, g.epi_plain);
    for (int i = 0; i < g.nseg; ++i) printf(" a%d=%llx/%llx/%llx", i, rec_p(g.a[i].base), rec_p(g.a[i].rows), rec_p(g.a[i].first_base));
    printf(" c=%llx/%llx/%llx", rec_p(g.c_in.base), rec_p(g.c_in.rows), rec_p(g.c_in.first_base));
    printf(" o=%llx co=%llx z=%llx go=%llx o2=%llx na=%llx", rec_p(g.out.base), rec_p(g.c_out.base), rec_p(g.zinit.base),
           rec_p(g.gates_out.base), rec_p(g.out2.base), rec_p(g.nact));
}
static void rec_launch(const char* form, int epi, unsigned gx, unsigned gy, unsigned gz, unsigned block, int lds, int want_img, int img_jobs,
                       const GemmBatch& b) {
    printf("L %s epi=%d grid=%u,%u,%u block=%u lds=%d img=%d/%d", form, epi, gx, gy, gz, block, lds, want_img, img_jobs);
    for (int j = 0; j < b.count; ++j) rec_job(b.g[j]);
    printf("\n");
}
static void rec_clear(const void* p, long long rows, long long cols, long long ld) {
    printf("C %llx rows=%lld cols=%lld ld=%lld\n", rec_p(p), rows, cols, ld);
}
static void rec_tn(const char* kernel, unsigned grid, unsigned block, int lds, const TnArgs& g) {
    printf("T %s grid=%u block=%u lds=%d nsplit=%d part=%llx colpart=%llx\n", kernel, grid, block, lds, g.nsplit, rec_p(g.part), rec_p(g.colpart));
}
static void rec_reduce(unsigned grid, int nz) { printf("R grid=%u nz=%d\n", grid, nz); }

// ---- the planner under test ----
static void run_gemm_case(const Keys& k, int epi, const GemmBatch& b) {
    static const char* const names[FORM_COUNT] = {"g128", "g128x2", "s128", "k32", "k64", "s256"};
    const GemmPlan plan = plan_gemm_launches(make_context(k), make_switches(k), epi, b);
    for (int i = 0; i < plan.count; ++i) {
        const GemmLaunchPlan& l = plan.launch[i];
        for (int j = 0; j < l.batch.count; ++j) {
            const GemmArgs& g = l.batch.g[j];
            if (l.clear_jobs >> j & 1)
                rec_clear(g.out.base + (long long)(g.step_imm * g.out.step_mul + g.out.step_add) * g.out.slot_stride, g.M, g.N, g.out.ld);
        }
        rec_launch(names[l.form], epi, l.grid_x, l.grid_y, l.grid_z, l.block, l.lds_bytes, l.want_image, l.image_jobs, l.batch);
    }
}
static void run_tn_case(const Keys& k, const TnArgs& t) {
    static const char* const names[TN_KERNEL_COUNT] = {"tn", "tns", "tn_part", "tns_part"};
    const bool ordered = key(k, "ordered_ws", 0);
    float* const ws = fake<float>(0, 4);
    const TnPlan p = plan_gemm_tn(make_context(k), make_switches(k), t, ordered);
    if (p.clear) rec_clear(t.C, t.Mstore, t.N, t.ldc);
    TnArgs gg = t;
    gg.nsplit = p.shares;
    if (ordered) { gg.part = ws; gg.colpart = ws + (size_t)p.nonempty * t.Mstore * t.N; }
    rec_tn(names[p.kernel], p.grid, p.block, p.lds_bytes, gg);
    if (p.reduce_grid) rec_reduce(p.reduce_grid, p.nonempty);
    printf("=> split=%d shares=%d nonempty=%d floats=%zu\n", p.kernel == TN_SPLIT || p.kernel == TN_SPLIT_PART, p.shares, p.nonempty,
           gemm_tn_plan_floats(plan_gemm_tn(make_context(k), make_switches(k), t, true), t));
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        std::string kind, name, rest;
        in >> kind >> name;
        std::getline(in, rest);
        printf("case %s\n", name.c_str());
        std::vector<std::string> groups;
        { std::istringstream gs(rest); std::string g; while (std::getline(gs, g, ';')) groups.push_back(g); }
        if (groups.empty()) groups.push_back("");
        const Keys k = parse_keys(groups[0], nullptr);
        if (kind == "T") { run_tn_case(k, make_tn(k)); continue; }
        const int epi = (int)key(k, "epi", 0);
        GemmBatch b{};
        for (size_t j = 1; j < groups.size() && b.count < GEMM_MAX_JOBS; ++j) b.g[b.count++] = make_job(epi, (int)j - 1, groups[j]);
        run_gemm_case(k, epi, b);
    }
    return 0;
}
