// Stand-alone driver of the decode path's persistent plans (cor_asv_ann_amd/csrc/persist_plan.h) for
// tests/test_persist_form_cases.py: reads cases on stdin, one per line, and prints the record of each plan on stdout.  Host code only.
//
//   E <name> d W residual deep B cus per_cu persistent split       an encoder pass (plan_persist_encode)
//   D <name> d W Vp C B cus per_cu persistent arithmetic           a greedy decode (plan_persist_decode)
#include "../cor_asv_ann_amd/csrc/persist_plan.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

using namespace casv;

int main() {
    static const char* const dec_reasons[] = {"ok", "off", "split_arithmetic", "cus", "depth", "lds", "not_worth"};
    static const char* const enc_reasons[] = {"ok", "off", "cus", "depth", "topology", "lds", "own", "not_worth"};
    static const char* const enc_forms[] = {"none", "chain", "split"};
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        std::string kind, name;
        int v[9] = {0};
        in >> kind >> name;
        for (int i = 0; i < 9; ++i) in >> v[i];
        if (!in || (kind != "E" && kind != "D")) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        printf("case %s\n", name.c_str());
        if (kind == "E") {
            const PersistEncPlan p = plan_persist_encode(PersistEncShape{v[0], v[1], v[2] != 0, v[3] != 0}, v[4], v[5], v[6], v[7], v[8] != 0);
            printf("E form=%s reason=%s grid=%d per_cu=%d own1=%d ownn=%d counters=%zu\n", enc_forms[p.form], enc_reasons[p.reason],
                   p.grid, p.per_cu, p.own1, p.ownn, p.counter_bytes);
        } else {
            const PersistDecPlan p = plan_persist_decode(PersistDecShape{v[0], v[1], v[2], v[3]}, v[4], v[5], v[6], v[7], v[8]);
            printf("D applies=%d reason=%s kmax=%d lda=%d lds=%zu per_cu=%d g_lstm=%d g_att=%d g_plain=%d counters=%zu\n", (int)p.applies,
                   dec_reasons[p.reason], p.kmax, p.lda, p.lds_bytes, p.per_cu, p.g_lstm, p.g_att, p.g_plain, p.counter_bytes);
        }
    }
    return 0;
}
