"""Models whose attention rows are steered by hand, and the table of searches run on them -- test infrastructure, importable
without a GPU (tests/test_steer_models.py on the CPU, tests/test_gpu_steered_attention.py on the device).

The tie models (tests/tie_models.py) turn the search's ORDER rules into bookkeeping; their attention tensors are zero, so the
alignment never moves and the rejection rule (oracle/decode.py decode_sequence_beam; csrc/beam_kernels.hip expand_row_scores and
new_node, fed by att_normalise's `apos` / `amax1`) is met only at source position 0 and in chains behind a rejection.  Here the
same two families get an attention that reads one channel of the encoder outputs and nothing else:

    att_Wa = 0, att_bUW = 0     the query adds nothing
    att_U[0, 0] = 1, else 0     u[s] = channel 0 of the encoder outputs at s
    att_va = G e_0, att_bv = 0  energy(s) = G tanh(enc_out[s, 0]),  G = 750

and channel 0 carries a "gate track": 0 at allowed source positions, -20 elsewhere.  An allowed position has energy exactly 0 and
weight exp(0) = 1; any other has energy about -750, whose exp is exactly 0 in float32 and in float64 (anything below -104 / -746
is; with G = 110 a float64 run kept weights of 1e-48).  The alignment row is then exactly fl(1/k) over the k allowed positions
inside the window and exactly 0 elsewhere, in both precisions and on the device whatever the last bit of its tanh(-20) is.  K and R
are zero in both families, so the context -- and the gate track in it -- never reaches the distribution: the search differs
from a tie model's only in where the alignment stands.  With k in {1, 2, 4, 8} the source position sum_s a[s] s is exact, so
halves are exact halves; with k <= 11 the float64 sum of fl32(1/k) s is exact in any order, so the device's `apos` and the
oracle's matmul agree to the bit for every k.

The encoder outputs are installed explicitly (casv_set_encoder_outputs; `search(m, source_seq, [enc_out] + states + [a0])`): the
states are the model's own, `a0` -- one-hot at a chosen position p, so that t' = p + 1 -- places the first window anywhere.

`tie_models.search` carries the trace of the rule (rej_mis_inside, rej_mis_outside, half_down, half_up, is1_by_attention,
is1_by_rejection, beyond_line, zero_source_row; mis_inside_max, mis_outside_min), the four flips REJECTION_RULES, the moved
thresholds THRESHOLD_RULES and the switch beyond_line='no_candidate'.
"""
import numpy as np

from oracle import ModelConfig
from tests import tie_models
from tests.tie_models import ALL, H, REJECTION_RULES, THRESHOLD_RULES, _u, search  # noqa: F401

G = 750.0
GATE_OFF = -20.0


def steered_weights(cfg, base):
    """`base` (a dict of tie_models.uniform_weights / held_weights) with the attention reading channel 0 of the encoder outputs."""
    w = {k: v.copy() for k, v in base.items()}
    for k in ('att_Wa', 'att_bUW', 'att_U', 'att_va', 'att_bv'):
        w[k] = np.zeros_like(w[k])
    w['att_U'][0, 0] = 1.0
    w['att_va'].reshape(-1)[0] = G
    return w


def track(T, allowed):
    """The gate track of one line: 0 at the allowed positions, GATE_OFF elsewhere."""
    t = np.full(T, GATE_OFF, np.float32)
    t[[s for s in allowed if 0 <= s < T]] = 0.0
    return t


class Case(tie_models.Case):
    """tie_models.Case plus, per line: `allowed` (the allowed source positions), `a0` (None: the zero row of the encoder, t' = 1;
    p: one-hot at p, t' = p + 1) and `zero_rows` (source positions whose input row is all zero, as a character of confidence 0
    is: no rejection candidate there).  window: ModelConfig.window / HipEngine(window_width=...).
    promises: trace key -> True (met at least once over the lines) or 0 (never met); flips: rule -> the output it changes, one of
    'text', 'rej', 'n_found', 'n_steps' (over all lines and results); the rules are tie_models.REJECTION_RULES and THRESHOLD_RULES."""

    def __init__(self, name, family, V, N, lines, allowed, a0=None, zero_rows=None, window=5, flips=None, width_out=4, open_end=False,
                 mis_inside=None, mis_outside=None, **kw):
        tie_models.Case.__init__(self, name, family, V, N, lines, width_out=width_out, **kw)
        self.open_end = open_end          # the lines without their '\n': the last source position holds a character
        if open_end:
            self.T = max(len(x) for x in lines)
        self.window = window
        self.cfg = ModelConfig(depth=tie_models.DEPTH, width=tie_models.WIDTH, voc_size=V, window=window)
        self.allowed = [list(a) for a in allowed]
        self.a0 = list(a0) if a0 is not None else [None] * len(lines)
        self.zero_rows = [list(z) for z in zero_rows] if zero_rows is not None else [[] for _ in lines]
        self.flips = flips or {}
        # the largest misalignment below 0.1 / the smallest not below it that an ordinary parent's row meets (trace: mis_inside_max,
        # mis_outside_min), over the lines; None: not promised
        self.mis_inside, self.mis_outside = mis_inside, mis_outside
        assert len(self.allowed) == len(self.a0) == len(self.zero_rows) == len(lines)
        self.beyond = bool(self.promises.get('beyond_line'))

    def weights(self, dtype=np.float32):
        return {k: v.astype(dtype) for k, v in steered_weights(self.cfg, tie_models.Case.weights(self)).items()}

    def texts(self):
        texts = tie_models.Case.texts(self)
        return [t[:-1] for t in texts] if self.open_end else texts

    def a0_rows(self):
        a = np.zeros((len(self.lines), self.T), np.float32)
        for j, p in enumerate(self.a0):
            if p is not None:
                a[j, p] = 1.0
        return a

    def inputs(self, m):
        """-> (enc_in (B,T,V) with the zero rows, idx (B,T) int32, src_rej (B,T) int32: -1 = an all-zero row)"""
        enc_in, _ = tie_models.Case.inputs(self, m)
        enc_in = enc_in.copy()
        for j, rows in enumerate(self.zero_rows):
            enc_in[j, rows] = 0
        idx = np.where(enc_in.any(axis=2), enc_in.argmax(axis=2), -1).astype(np.int32)
        return enc_in, idx, idx.copy()

    def encoder_outputs(self, m):
        """-> [enc_out (B,T,C), h1, c1, ..., a0]: the model's own encoding of the lines, channel 0 replaced by the gate tracks."""
        dt = m.weights['E'].dtype
        enc = m.encode(tie_models.Case.inputs(self, m)[0])
        enc_out = enc[0].copy()
        for j, allowed in enumerate(self.allowed):
            enc_out[j, :, 0] = track(self.T, allowed).astype(dt)
        return [enc_out] + list(enc[1:-1]) + [self.a0_rows().astype(dt)]

    def expected_row(self, j, tprime):
        """The alignment row of line j for a window around t' (a float32), in float32: fl32(1/k) on the allowed positions inside."""
        s = np.arange(self.T)
        inside = np.abs(np.float32(tprime) - s.astype(np.float32)) <= np.float32(self.window)
        inside &= np.isin(s, self.allowed[j])
        k = int(inside.sum())
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(inside, np.float32(1) / np.float32(k), np.float32(0) / np.float32(k)).astype(np.float32)


def run_search(case, dtype=np.float32, rules=()):
    """-> per line (results, stats, trace) of `search` on the steered encoder outputs."""
    m = case.model(dtype)
    enc_in = case.inputs(m)[0]
    enc = case.encoder_outputs(m)
    out = []
    for j in range(len(case.lines)):
        trace = {}
        res, stats = search(m, enc_in[j], [e[j:j + 1] for e in enc], rules, trace, case.lm,
                            beyond_line='no_candidate' if case.beyond else None)
        out.append((res, stats, trace))
    return out


def _line(n, V, start=2):
    """n distinct-neighbour characters: consecutive vocabulary indices from `start`, wrapping inside 2..V-1."""
    return [2 + (start - 2 + i) % (V - 2) for i in range(n)]


def _holes(T, *holes):
    return [s for s in range(T) if s not in holes]


def _onehot_track(T, first, gap=11):
    """One allowed position per window of width 5: `first`, first + gap, ..."""
    return list(range(first, T, gap))


T30, L30 = 30, _line(29, 32)
T24, L24 = 24, _line(23, 16)
Z0 = [[0]]         # source position 0 has a zero row: no rejection candidate behind the root, so that no result is the plain copy of
#                    the source line that the chain of rejections from position 0 gives, and every returned string shows where the
#                    steered rule put its first rejection
IS1 = {'is1_ignored': 'text', 'is1_from_attention_row': 'text'}
CASES = [
    # --- dense tracks: the window full, the position walks on by exactly 1 a step
    Case('dense_root_n1', 'uniform', 16, 1, [L24], [range(T24)], width_out=1, is1_by_rejection=True, is1_by_attention=0, flips=IS1),
    Case('dense_mid_n4', 'uniform', 32, 4, [L30], [range(T30)], a0=[10], zero_rows=Z0, rej_mis_inside=True, rej_mis_outside=0,
         is1_by_rejection=True, zero_source_row=True, flips=IS1),
    Case('dense_mid_n8', 'uniform', 32, 8, [L30, L30[:18]], [range(T30), range(T30)], a0=[7, 3], zero_rows=[[0], [0]],
         rej_mis_inside=True, rej_mis_outside=0, flips=IS1),
    Case('dense_mid_n64', 'uniform', 16, 64, [L24], [range(T24)], a0=[6], zero_rows=Z0, rejection=_u(16), threshold_in=ALL,
         rej_mis_inside=True, is1_by_rejection=True, flips={'mis_not_tested': 'rej'}),
    # --- the misalignment next to 0.1: 2/21 inside; 1/9 and 1/8 outside (1/11 cannot occur: see the note below the table)
    Case('mis_2_21', 'uniform', 32, 4, [L30], [_holes(T30, 8, 9, 13)], a0=[10], zero_rows=Z0, rej_mis_inside=True, rej_mis_outside=True,
         mis_inside=2 / 21, flips={'mis_not_tested': 'text', 'mis_below_0_09': 'text'}),
    Case('mis_1_9', 'uniform', 32, 4, [L30], [[5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 20, 22, 23, 26, 27, 29]], a0=[8], zero_rows=Z0,
         rej_mis_inside=True, rej_mis_outside=True, mis_outside=1 / 9, flips={'mis_not_tested': 'text', 'mis_below_0_13': 'text'}),
    Case('mis_1_8', 'uniform', 32, 4, [L30], [_holes(T30, 8, 10, 19)], a0=[10], zero_rows=Z0, rej_mis_inside=0, rej_mis_outside=True,
         is1_by_rejection=0, mis_outside=1 / 8, flips={'mis_not_tested': 'n_found', 'mis_below_0_13': 'n_found'}),
    # --- exact halves: 15.5 -> 16.5 -> 16 (down to the even neighbour), 14.5 -> 15.5 -> 16 (up to it)
    Case('half_down', 'uniform', 32, 4, [L30], [[15, 16, 17, 18]], a0=[10], zero_rows=Z0, half_down=True, half_up=0, rej_mis_inside=True,
         flips={'round_half_up': 'text'}),
    Case('half_up', 'uniform', 32, 4, [L30], [[14, 15, 16, 17]], a0=[9], zero_rows=Z0, half_up=True, half_down=0, rej_mis_inside=True),
    Case('halves_n8', 'uniform', 32, 8, [L30, L30[:22]], [[15, 16, 17, 18], [14, 15, 16, 17]], a0=[10, 9], zero_rows=[[0], [0]],
         half_down=True, half_up=True, flips={'round_half_up': 'rej'}),
    Case('halves_n64', 'uniform', 16, 64, [L24, L24[:20]], [[11, 12, 13, 14], [10, 11, 12, 13]], a0=[6, 5], zero_rows=[[0], [0]],
         half_down=True, half_up=True, flips={'round_half_up': 'text'}),
    Case('half_down_held', H(4), 24, 4, [_line(29, 24)], [[15, 16, 17, 18]], a0=[10], zero_rows=Z0, width_in=3, threshold_in=ALL,
         half_down=True, flips={'round_half_up': 'text', 'mis_not_tested': 'text'}),
    Case('half_up_lm', 'uniform', 64, 4, [_line(29, 64)], [[14, 15, 16, 17]], a0=[9], zero_rows=Z0, lm=True, half_up=True),
    # --- a zero source row at the steered position: no candidate, nothing ever finishes
    Case('half_zero_row', 'uniform', 32, 4, [L30], [[15, 16, 17, 18]], a0=[10], zero_rows=[[0, 16]], zero_source_row=True, half_down=True,
         is1_by_rejection=0, flips={'round_half_up': 'n_found'}),
    # --- one allowed position per window: one-hot by attention, the position stalls, the record walks on by rejections
    Case('onehot_stall', 'uniform', 32, 4, [L30], [[14, 25]], a0=[10], zero_rows=Z0, is1_by_attention=True, is1_by_rejection=True,
         rej_mis_inside=0, rej_mis_outside=0, flips={'is1_ignored': 'text'}),
    Case('onehot_n1', 'uniform', 16, 1, [L24], [[9, 20]], a0=[5], zero_rows=Z0, width_out=1, is1_by_attention=True,
         flips={'is1_ignored': 'text'}),
    Case('onehot_n64', 'uniform', 16, 64, [L24], [[9, 20]], a0=[5], zero_rows=Z0, width_in=3, threshold_in=ALL, is1_by_attention=True,
         flips={'is1_ignored': 'text'}),
    Case('onehot_held', H(4), 24, 8, [_line(29, 24)], [[14, 25]], a0=[10], zero_rows=Z0, width_in=3, threshold_in=ALL, width_out=1,
         is1_by_attention=True, flips={'is1_ignored': 'text'}),
    # --- the source position beyond the line: the last source character is no '\n', so a rejection at T - 1 is expanded; the one
    #     allowed position is T - 1
    Case('beyond_by_rejection', 'uniform', 16, 8, [L24], [range(T24 - 1)], open_end=True, width_out=16, beyond_line=True,
         is1_by_rejection=True),
    Case('beyond_by_attention', 'uniform', 16, 4, [L24], [[22]], a0=[20], zero_rows=Z0, open_end=True, beyond_line=True,
         is1_by_attention=True, is1_by_rejection=0),
    # --- the first window at the end of the line, partly off it
    Case('a0_end', 'uniform', 32, 4, [L30], [[25]], a0=[29], zero_rows=Z0, is1_by_attention=True, flips={'is1_ignored': 'text'}),
    # --- window widths 1 to 4: dense and one-hot
    Case('dense_w1', 'uniform', 32, 4, [L30], [range(T30)], a0=[10], zero_rows=Z0, window=1, rej_mis_inside=True, flips=IS1),
    Case('dense_w2', 'uniform', 32, 4, [L30], [range(T30)], a0=[10], zero_rows=Z0, window=2, rej_mis_inside=True, flips=IS1),
    Case('dense_w3', 'uniform', 32, 4, [L30], [range(T30)], a0=[8], zero_rows=Z0, window=3, rej_mis_inside=True, flips=IS1),
    Case('dense_w4', 'uniform', 32, 4, [L30], [range(T30)], a0=[10], zero_rows=Z0, window=4, rej_mis_inside=True, flips=IS1),
    Case('onehot_w1', 'uniform', 32, 4, [L30], [_onehot_track(T30, 11, 3)], a0=[10], zero_rows=Z0, window=1, is1_by_attention=True,
         flips={'is1_ignored': 'text'}),
    Case('onehot_w2', 'uniform', 32, 4, [L30], [_onehot_track(T30, 12, 5)], a0=[10], zero_rows=Z0, window=2, is1_by_attention=True,
         flips={'is1_ignored': 'text'}),
    Case('onehot_w3', 'uniform', 32, 8, [L30], [_onehot_track(T30, 13, 7)], a0=[10], zero_rows=Z0, window=3, is1_by_attention=True,
         flips={'is1_ignored': 'text'}),
    Case('onehot_w4', 'uniform', 32, 64, [L30], [_onehot_track(T30, 14, 9)], a0=[10], zero_rows=Z0, window=4, is1_by_attention=True,
         flips={'is1_ignored': 'text'}),
]
# A misalignment of exactly 1/11 cannot occur on such rows: it needs a mean over k = 11 positions, and a window holds 11 positions only
# around an integer t' with all of them allowed -- then the mean IS t' and the misalignment 0.  Of all patterns of up to four
# forbidden positions in two consecutive windows of width 5, the largest misalignment below the threshold is 2/21 (k = 7 then 9).
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
