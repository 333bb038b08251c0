// Stand-alone host check of the Keras <-> packed table (cor_asv_ann_amd/csrc/keras_table.h): no device, its own main.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Wall -Werror tests/keras_table_check.cpp -o check && ./check
// For depth 1, depth 2, depth 2 + deep_bidirectional_encoder and depth 2 + bridge_dense at W = 32, V = 7: every Keras tensor gets
// all-distinct values (0, 1, 2, ... over the whole model), is packed entry by entry, and
//   - the packed tensors are numbered 0 .. n-1 without a gap, each named by exactly one entry (an LSTM's triple by its three members),
//     and every packed element receives a Keras value exactly once: the images of different entries do not overlap and leave no hole;
//   - unpacking every entry gives the Keras tensors back exactly;
//   - packing one member of an LSTM with the other two read back from the packed triple (what a set does) changes only that member.
// Prints one line per configuration; exit status 1 and the first difference on a failure.
#include "../cor_asv_ann_amd/csrc/keras_table.h"

#include <cstdio>
#include <cstring>

using namespace casv;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (!failures++) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static size_t packed_count(int W, const KerasEntry& e, int j) {
    if (!e.lstm()) return e.count();
    return j == 0 ? (size_t)4 * W * e.kx : j == 1 ? (size_t)4 * W * (e.kctx + W) : (size_t)4 * W;
}

static void check(const char* what, int W, int V, int D, bool deep, bool bridge) {
    const int C = (D == 1 || deep) ? 2 * W : W;
    const std::vector<KerasEntry> table = keras_table(W, V, C, D, deep, bridge);
    KerasView keras;
    float next = 0.f;
    size_t total = 0;
    for (const KerasEntry& e : table) {
        CHECK(!keras.count(e.name), "%s: name %s twice", what, e.name.c_str());
        std::vector<float>& v = keras[e.name];
        v.resize(e.count());
        for (float& x : v) x = next++;
        total += e.count();
    }
    CHECK(total < (1u << 24), "%s: %zu values are not all distinct in float32", what, total);
    // pack: every packed tensor from exactly one entry (or one LSTM triple)
    std::map<int, std::vector<float>> packed;
    std::map<int, std::string> owner;
    for (const KerasEntry& e : table) {
        std::vector<float> p[3];
        keras_pack(W, e, keras, p);
        for (int j = 0; j < e.parts(); ++j) {
            CHECK(p[j].size() == packed_count(W, e, j), "%s: %s part %d has %zu elements", what, e.name.c_str(), j, p[j].size());
            const std::string who = e.lstm() ? e.group : e.name;
            if (owner.count(e.part[j])) {
                CHECK(owner[e.part[j]] == who, "%s: packed tensor %d belongs to %s and %s", what, e.part[j], owner[e.part[j]].c_str(), who.c_str());
                CHECK(packed[e.part[j]] == p[j], "%s: %s packs part %d differently from its layer's other members", what, e.name.c_str(), j);
            }
            owner[e.part[j]] = who;
            packed[e.part[j]] = p[j];
        }
    }
    std::vector<char> seen(total, 0);
    size_t packed_total = 0;
    int index = 0;
    for (auto& kv : packed) {
        CHECK(kv.first == index, "%s: packed tensors are not numbered without a gap at %d", what, index);
        ++index;
        packed_total += kv.second.size();
        for (float x : kv.second) {
            const size_t i = (size_t)x;
            CHECK(x >= 0.f && i < total && (float)i == x, "%s: packed tensor %d holds %g, no Keras value", what, kv.first, (double)x);
            if (i < total) { CHECK(!seen[i], "%s: Keras value %zu lies in two packed places", what, i); seen[i] = 1; }
        }
    }
    CHECK(packed_total == total, "%s: %zu packed elements for %zu Keras values", what, packed_total, total);
    // unpack: exact round trip, entry by entry
    for (const KerasEntry& e : table) {
        std::vector<float> p[3];
        for (int j = 0; j < e.parts(); ++j) p[j] = packed[e.part[j]];
        KerasView back;
        keras_unpack(W, e, p, back);
        CHECK(back.count(e.name) && back[e.name] == keras[e.name], "%s: %s does not come back from its packed image", what, e.name.c_str());
        CHECK((int)back.size() == e.parts(), "%s: unpacking %s gave %zu tensors", what, e.name.c_str(), back.size());
        for (auto& kv : back) CHECK(kv.second == keras[kv.first], "%s: unpacking %s changed %s", what, e.name.c_str(), kv.first.c_str());
    }
    // a set: new values for one tensor, an LSTM member packed again with the other two as the packed triple holds them
    for (const KerasEntry& e : table) {
        std::vector<float> p[3];
        for (int j = 0; j < e.parts(); ++j) p[j] = packed[e.part[j]];
        KerasView view;
        if (e.lstm()) keras_unpack(W, e, p, view);
        std::vector<float> fresh(e.count());
        for (size_t i = 0; i < fresh.size(); ++i) fresh[i] = -1.f - (float)i;
        view[e.name] = fresh;
        keras_pack(W, e, view, p);
        KerasView back;
        keras_unpack(W, e, p, back);
        for (auto& kv : back)
            CHECK(kv.second == (kv.first == e.name ? fresh : keras[kv.first]), "%s: setting %s left %s wrong", what, e.name.c_str(), kv.first.c_str());
    }
    printf("%s: %zu entries, %d packed tensors, %zu values: %s\n", what, table.size(), index, total, failures ? "FAILED" : "ok");
    for (const KerasEntry& e : table) printf("  %s %d %d\n", e.name.c_str(), e.rows, e.cols);        // (the test compares these with weight_shapes)
}

int main() {
    const int W = 32, V = 7;
    check("depth 1", W, V, 1, false, false);
    check("depth 2", W, V, 2, false, false);
    check("depth 2, deep_bidirectional_encoder", W, V, 2, true, false);
    check("depth 2, bridge_dense", W, V, 2, false, true);
    return failures ? 1 : 0;
}
