// The Keras view of the train step's packed tensors, stated once: one entry per Keras tensor name says how its values are stored.
//   PLAIN       verbatim in packed tensor part[0]
//   TRANSPOSED  [rows][cols] stored [cols][rows] in part[0]: att_U as [W][C], att_Wa and the bridge kernels as [W][W]
//   LSTM_K/R/B  member K (kx + kctx, 4W) / R (W, 4W) / b (4W) of a layer whose three tensors are stored together as the triple
//               Wx [4W][kx] = part[0], Wr [4W][kctx + W] = part[1], bias [4W] = part[2], rows in the gate-interleaved order of gemm.hip
// Packed tensors are numbered in the order the entries first name them; build_state (train_state.hip) creates them by walking the
// table, the accessors find a name in it.  Plain host code: nothing here touches the device (tests/keras_table_check.cpp).
#pragma once
#include <map>
#include <string>
#include <vector>

namespace casv {

using KerasView = std::map<std::string, std::vector<float>>;

struct KerasEntry {
    enum Form { PLAIN, TRANSPOSED, LSTM_K, LSTM_R, LSTM_B };
    std::string name;
    std::string group;                  // the layer or bridge the tensor belongs to ("": none) -- what a frozen prefix names
    Form form = PLAIN;
    int rows = 1, cols = 0;             // the Keras tensor [rows][cols] (a vector: one row)
    int part[3] = {-1, -1, -1};
    int kx = 0, kctx = 0;               // LSTM: width of the input / of the context that joins the recurrent part (the attention cell's)
    bool encoder = false; int dir = 0;  // LSTM: an encoder layer; 0 forward, 1 backward in time
    bool lstm() const { return form >= LSTM_K; }
    int parts() const { return lstm() ? 3 : 1; }
    size_t count() const { return (size_t)rows * cols; }
    std::string packed_name(int j) const { return lstm() ? group + (j == 0 ? "_Wx" : j == 1 ? "_Wr" : "_b") : form == TRANSPOSED ? name + "T" : name; }
};

inline int gate_row(int W, int u, int g) { return (u / 32) * 128 + g * 32 + (u % 32); }

// Keras (K (kin,4W), R (W,4W), b) -> Wx [4W][kx], Wr [4W][kr], bias [4W]; top: K rows [W, W+C) join the recurrent part
inline void pack_train_lstm(int W, int kx, int kctx, const std::vector<float>& K, const std::vector<float>& R,
                            const std::vector<float>& b, std::vector<float>& wx, std::vector<float>& wr, std::vector<float>& bias) {
    const int kr = kctx + W;
    wx.assign((size_t)4 * W * kx, 0.f); wr.assign((size_t)4 * W * kr, 0.f); bias.assign(4 * W, 0.f);
    for (int u = 0; u < W; ++u)
        for (int g = 0; g < 4; ++g) {
            const int n = gate_row(W, u, g), col = g * W + u;
            for (int k = 0; k < kx; ++k) wx[(size_t)n * kx + k] = K[(size_t)k * 4 * W + col];
            for (int k = 0; k < kctx; ++k) wr[(size_t)n * kr + k] = K[(size_t)(kx + k) * 4 * W + col];
            for (int k = 0; k < W; ++k) wr[(size_t)n * kr + kctx + k] = R[(size_t)k * 4 * W + col];
            bias[n] = b[col];
        }
}
inline void unpack_train_lstm(int W, int kx, int kctx, const std::vector<float>& wx, const std::vector<float>& wr,
                              const std::vector<float>& bias, std::vector<float>& K, std::vector<float>& R, std::vector<float>& b) {
    const int kr = kctx + W;
    K.assign((size_t)(kx + kctx) * 4 * W, 0.f); R.assign((size_t)W * 4 * W, 0.f); b.assign(4 * W, 0.f);
    for (int u = 0; u < W; ++u)
        for (int g = 0; g < 4; ++g) {
            const int n = gate_row(W, u, g), col = g * W + u;
            for (int k = 0; k < kx; ++k) K[(size_t)k * 4 * W + col] = wx[(size_t)n * kx + k];
            for (int k = 0; k < kctx; ++k) K[(size_t)(kx + k) * 4 * W + col] = wr[(size_t)n * kr + k];
            for (int k = 0; k < W; ++k) R[(size_t)k * 4 * W + col] = wr[(size_t)n * kr + kctx + k];
            b[col] = bias[n];
        }
}

// in [rows][cols] -> out [cols][rows]
inline std::vector<float> transposed(const std::vector<float>& in, int rows, int cols) {
    std::vector<float> out((size_t)rows * cols);
    for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) out[(size_t)c * rows + r] = in[(size_t)r * cols + c];
    return out;
}

// The table of a model: E; the LSTM layers enc1_fw, enc1_bw, enc2.. (deep: encN_fw, encN_bw), dec1..decD; the attention; the bridges.
inline std::vector<KerasEntry> keras_table(int W, int V, int C, int D, bool deep, bool bridge) {
    std::vector<KerasEntry> t;
    int next = 0;
    auto one = [&](const std::string& name, KerasEntry::Form form, int rows, int cols, const std::string& group = "") {
        KerasEntry e;
        e.name = name; e.group = group; e.form = form; e.rows = rows; e.cols = cols; e.part[0] = next++;
        t.push_back(e);
    };
    auto lstm = [&](const std::string& layer, int kx, int kctx, bool encoder, int dir) {
        KerasEntry e;
        e.group = layer; e.kx = kx; e.kctx = kctx; e.encoder = encoder; e.dir = dir;
        for (int j = 0; j < 3; ++j) e.part[j] = next++;
        e.name = layer + "_K"; e.form = KerasEntry::LSTM_K; e.rows = kx + kctx; e.cols = 4 * W; t.push_back(e);
        e.name = layer + "_R"; e.form = KerasEntry::LSTM_R; e.rows = W; t.push_back(e);
        e.name = layer + "_b"; e.form = KerasEntry::LSTM_B; e.rows = 1; t.push_back(e);
    };
    one("E", KerasEntry::PLAIN, V, W);
    lstm("enc1_fw", W, 0, true, 0); lstm("enc1_bw", W, 0, true, 1);
    for (int n = 2; n <= D; ++n) {
        const std::string layer = "enc" + std::to_string(n);
        if (deep) { lstm(layer + "_fw", 2 * W, 0, true, 0); lstm(layer + "_bw", 2 * W, 0, true, 1); }   // every layer bidirectional, 2W-wide inputs (seq2seq.py:273-276)
        else lstm(layer, n == 2 ? 2 * W : W, 0, true, 0);
    }
    for (int n = 1; n <= D; ++n) lstm("dec" + std::to_string(n), W, n == D ? C : 0, false, 0);
    one("att_U", KerasEntry::TRANSPOSED, C, W);
    one("att_Wa", KerasEntry::TRANSPOSED, W, W);
    one("att_bUW", KerasEntry::PLAIN, 1, W);
    one("att_va", KerasEntry::PLAIN, 1, W);
    one("att_bv", KerasEntry::PLAIN, 1, 1);
    for (int n = 1; n <= D && bridge; ++n)          // bridge_dense (seq2seq.py:299-301): per encoder layer the Dense of h, then of c
        for (const char* s : {"_h", "_c"}) {
            const std::string b = "bridge" + std::to_string(n) + s;
            one(b + "_K", KerasEntry::TRANSPOSED, W, W, b);
            one(b + "_b", KerasEntry::PLAIN, 1, W, b);
        }
    return t;
}

inline const KerasEntry* keras_find(const std::vector<KerasEntry>& table, const std::string& name) {
    for (const KerasEntry& e : table) if (e.name == name) return &e;
    return nullptr;
}

// Keras -> packed: p[j] = the image of packed tensor e.part[j] (an LSTM member: the triple, from the layer's three tensors in `in`)
inline void keras_pack(int W, const KerasEntry& e, const KerasView& in, std::vector<float> p[3]) {
    if (e.lstm()) pack_train_lstm(W, e.kx, e.kctx, in.at(e.group + "_K"), in.at(e.group + "_R"), in.at(e.group + "_b"), p[0], p[1], p[2]);
    else p[0] = e.form == KerasEntry::TRANSPOSED ? transposed(in.at(e.name), e.rows, e.cols) : in.at(e.name);
}
// packed -> Keras: out[e.name] (an LSTM member comes with its layer's other two: the triple holds them together)
inline void keras_unpack(int W, const KerasEntry& e, const std::vector<float> p[3], KerasView& out) {
    if (e.lstm()) unpack_train_lstm(W, e.kx, e.kctx, p[0], p[1], p[2], out[e.group + "_K"], out[e.group + "_R"], out[e.group + "_b"]);
    else out[e.name] = e.form == KerasEntry::TRANSPOSED ? transposed(p[0], e.cols, e.rows) : p[0];
}

}  // namespace casv
