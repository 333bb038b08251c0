// Stand-alone driver of the train step's persistent-launch plan (cor_asv_ann_amd/csrc/train_plan.h) for
// tests/test_train_form_cases.py: reads cases on stdin and prints the record of each on stdout.  Host code only.
//
//   K                                                             the header's constants and width lists
//   G <kind> W C B U jobs cus per_cu                              one shape rule (train_form_grid)
//   S <name> persistent deterministic backoff cus nsites          one step (TrainStepPlan), followed by nsites lines, in the step's order:
//     <kind> W C B U jobs per_cu plain T defer split split_off rows_fit
//   B count W rows0 N0 rows1 N1                                   one fused backward step (bwd_step_plan; count 1: rows1 and N1 are ignored)
#include "../cor_asv_ann_amd/csrc/train_plan.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace casv;

static const char* const kinds[TRAIN_KINDS] = {"rec", "rec_bwd", "cell", "cell_bwd"};

static int kind_of(const std::string& s) {
    for (int k = 0; k < TRAIN_KINDS; ++k) if (s == kinds[k]) return k;
    return -1;
}

static int bad(const std::string& line) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        std::string what, name;
        in >> what;
        if (what == "K") {
            printf("constants row_block=%d cap=%d min_cus=%d defer_max_t=%d\n", TRAIN_ROW_BLOCK, TRAIN_LAUNCH_CAP, TRAIN_MIN_CUS, ATTN_DEFER_MAX_T);
            for (int k = 0; k < TRAIN_KINDS; ++k) {
                printf("kind %s per_cu=%d counters=%d widths=", kinds[k], TRAIN_BLOCKS_PER_CU[k], TRAIN_COUNTERS_PER_ROW_BLOCK[k]);
                for (int nt = 0; nt <= 64; ++nt) if (train_has_width((TrainKind)k, nt)) printf("%d,", nt);
                printf("\n");
            }
        } else if (what == "G") {
            int v[7] = {0};
            in >> name;
            for (int& x : v) in >> x;
            const int k = kind_of(name);
            if (!in || k < 0) return bad(line);
            printf("grid=%d\n", train_form_grid((TrainKind)k, TrainShape{v[0], v[1], v[2], v[3], v[4]}, v[5], v[6]));
        } else if (what == "S") {
            int g[5] = {0};
            in >> name;
            for (int& x : g) in >> x;
            if (!in) return bad(line);
            printf("case %s\n", name.c_str());
            const TrainGate gate{g[0], g[1] != 0, g[2] != 0, g[3]};
            TrainStepPlan plan;
            int B = 0;
            for (int i = 0; i < g[4]; ++i) {
                if (!std::getline(std::cin, line)) return bad("a step ends early");
                std::istringstream sin(line);
                int v[12] = {0};
                sin >> name;
                for (int& x : v) sin >> x;
                const int k = kind_of(name);
                if (!sin || k < 0) return bad(line);
                const TrainSite site{(TrainKind)k, TrainShape{v[0], v[1], v[2], v[3], v[4]}, v[5], v[6] != 0, v[7], TrainSwitches{v[8], v[9] != 0},
                                     v[10] != 0, v[11] != 0};
                const TrainLaunch p = plan.next(gate, site);
                printf("site kind=%s persistent=%d capped=%d grid=%d nt=%d slot=%d offset=%zu counters=%zu defer=%d split=%d\n", kinds[k],
                       (int)p.persistent, (int)p.capped, p.grid, p.nt, p.slot, p.slot_offset, p.counter_bytes, p.defer, p.split_a);
                B = v[2];
            }
            printf("step count=%d slot_bytes=%zu\n", plan.launches, train_slot_bytes(B));
        } else if (what == "B") {
            int v[6] = {0};
            for (int& x : v) in >> x;
            if (!in || v[0] < 1 || v[0] > 2) return bad(line);
            const int rows[2] = {v[2], v[4]}, N[2] = {v[3], v[5]};
            const BwdStepPlan p = bwd_step_plan(rows, N, v[0], v[1]);
            printf("bwd_step blocks=%d ksplit=%d gper=%d\n", p.blocks, p.ksplit, p.gper);
        } else return bad(line);
    }
    return 0;
}
