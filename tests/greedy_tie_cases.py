"""Models on which the greedy decode's pick is decided by its bookkeeping alone, and the table of decodes run on them -- test
infrastructure, importable without a GPU (tests/test_greedy_tie_cases.py on the CPU, tests/test_gpu_greedy_ties.py on the device).

The pick of a character from a softmax row exists four times on the device (csrc/decode_kernels.hip softmax_kernel, one wave per row,
entry v in lane v & 63; csrc/persist.hip row_stats_quarter<true> at V = Vp = 256 and row_stats_quarter<false> at V <= 256, four rows
per wave, entry v in lane v & 15 of its quarter, slot v >> 4; row_stats at V > 256, one row per wave over the permuted staged row).
Its rules (oracle/decode.py decode_batch_greedy / decode_sequence_greedy):

mode 0    np.nanargmax(scores[1:]) + 1: index 0 is never picked, the first maximum wins
mode 1    np.nanargmax over all V; if that is index 0 -- it is >= every later entry -- NaN is written over p[0], STAYS in the fed-back
          distribution, and the pick is taken again over the rest
ties      towards the lower index, inside a lane, across lanes, across the butterflies
all NaN   index 1 with a NaN probability; in mode 1 the line raises if that happens before its '\\n'
padding   columns V .. Vp-1 are exact zeros and never candidates

Families: *uniform* (tests/tie_models.py: every tensor zero) and *tied* (`tied_weights`: the held-state model with chosen E rows made
identical).  All units of the held h hold one value, so a logit is that value times the sum of its E row: set 0 gets the row with the
largest sum plus a boost (it wins where h > 0), set 1 the row with the smallest sum minus a boost (it wins where h < 0).  `explicit`
cases install encoder outputs whose decoder states are constant per row and differ between rows (`explicit_outputs`), one row
optionally NaN.

`pick` / `greedy` restate the rule with a switch for each of five mutations; tests/test_greedy_tie_cases.py shows that with no switch
they are the oracle's functions and that every switch changes an expected output of the table.
"""
import numpy as np

from oracle import ModelConfig, make_vocabulary, vectorize_lines
from oracle.decode import OracleModel, decode_batch_greedy, decode_sequence_greedy
from tests.tie_models import DEPTH, WIDTH, UNMAPPED, uniform_weights, held_weights

BOOST = 0.5          # per entry of the top row: 16 on its sum, far above every gap of the table
GAP = 0.01           # per entry: a strict second place, 0.32 below on the row sum
SAT = 64.0           # E x 64: every logit gap of the table is beyond 150


# ------------------------------------------------------------------------------------------------------------------ models
def _in_one_entry(row):
    """The row with its whole sum in entry 0.  All units of the held h hold one value, so the logit is that value times the row
    sum either way -- but as ONE product plus zeros it has the same bits in every summation order: BLAS kernels round the last
    columns of a matrix differently from the others (sgemm gave identical rows 1 and V - 1 of V = 255 probabilities 16 ulps
    apart), and a tie must be exact in the oracle, in both its precisions, before it can pin the device."""
    out = np.zeros_like(row)
    out[0] = np.float32(row.astype(np.float64).sum())
    return out


def tied_weights(cfg, sets, scale=1.0, gaps=None, boost=BOOST):
    """The held-state model (every index its own E row) with the rows of set 0 replaced by the row of the largest sum + boost, those
    of an optional set 1 by the row of the smallest sum - boost; gaps {index: amount}: that index gets the top row with `amount`
    subtracted from every entry (a strict second place); each of these rows carries its sum in one entry (_in_one_entry); scale
    multiplies E."""
    w = held_weights(cfg, group=1, split01=False)
    E = w['E'].copy()
    sums = E.astype(np.float64).sum(axis=1)
    top = E[int(np.argmax(sums))] + np.float32(boost)
    bottom = E[int(np.argmin(sums))] - np.float32(boost)
    assert len(sets) <= 2
    for row, members in zip((top, bottom), sets):
        for v in members:
            E[v] = _in_one_entry(row)
    for v, amount in (gaps or {}).items():
        E[v] = _in_one_entry(top - np.float32(amount))
    w['E'] = (E * np.float32(scale)).astype(np.float32)
    return w


def held_h(T):
    """The value every unit of the top decoder layer's h holds on the held-state model after an encoder pass over T positions
    (float64): the encoder's cells see zero K and R and biases 0.7, the decoder's output gate bias 1."""
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    c = 0.0
    for _ in range(T):
        c = sig(0.7) * c + sig(0.7) * np.tanh(0.7)
    return sig(1.0) * np.tanh(c)


# row r of an explicit batch holds c = h = 0.2 + 0.15 r in every layer; these rows are negative (set 1 wins there)
NEGATIVE_ROWS = {2: -0.5, 30: -1.3}


def row_values(B):
    return np.array([NEGATIVE_ROWS.get(r, 0.2 + 0.15 * r) for r in range(B)])


def explicit_outputs(enc, nan_row=None):
    """enc = [enc_out, h1, c1, ..., a0] of the model's own encoder -> the same with every decoder state constant per row
    (row_values), row `nan_row`'s c NaN in every layer."""
    B = enc[0].shape[0]
    out = [enc[0]]
    for k, st in enumerate(enc[1:-1]):
        v = np.repeat(row_values(B)[:, None], st.shape[1], axis=1).astype(st.dtype)
        if nan_row is not None and k % 2 == 1:
            v[nan_row] = np.nan
        out.append(v)
    return out + [enc[-1]]


# ------------------------------------------------------------------------------------------------------------------ forms
def greedy_form(V):
    """Which row-statistics form persist_decode_kernel takes (csrc/persist.hip: `if (V == 256 && Vp == 256) ... else if (V <= 256) ...
    else`), with Vp = (V + 31) & ~31 as casv_model_create pads it (csrc/engine.hip)."""
    Vp = (V + 31) & ~31
    if V == 256 and Vp == 256:
        return 'quarter_full'
    return 'quarter' if V <= 256 else 'wave'


# ------------------------------------------------------------------------------------------------------------------ the rule
RULES = ('tie_high', 'zero_in_mode0', 'zero_gt', 'no_writeback', 'writeback_mode0')


def pick(scores, mode, rules=()):
    """One row.  -> (index, probability, nan0, all_nan): nan0 = NaN goes over entry 0 of the fed-back row; all_nan = no candidate
    is a number (numpy raises; the device reports index 1 with a NaN probability).
    rules  'tie_high'         ties go to the higher index
           'zero_in_mode0'    index 0 is a candidate in mode 0
           'zero_gt'          index 0 wins only if strictly greater than every later entry
           'no_writeback'     the NaN is not fed back
           'writeback_mode0'  the NaN is also written in mode 0"""
    assert set(rules) <= set(RULES)

    def argmax(lo):
        cand = scores[lo:]
        ok = ~np.isnan(cand)
        if not ok.any():
            return None
        hits = np.flatnonzero(ok & (cand == cand[ok].max()))
        return lo + int(hits[-1] if 'tie_high' in rules else hits[0])

    k = argmax(1)
    if k is None:
        return 1, scores.dtype.type(np.nan), False, True
    p0 = scores[0]
    zero_wins = bool(p0 > scores[k] if 'zero_gt' in rules else p0 >= scores[k])       # (False for a NaN p0)
    if mode == 0:
        if 'zero_in_mode0' in rules and zero_wins:
            k = 0
        return k, scores[k], zero_wins and 'writeback_mode0' in rules, False
    return k, scores[k], zero_wins and 'no_writeback' not in rules, False


def _loop(m, enc, mode, rules):
    attended, states = enc[0], list(enc[1:])
    R, T = attended.shape[:2]
    S, V = 2 * T, m.voc_size
    dt = m.weights['E'].dtype
    u = attended @ m.weights['att_U']
    target = np.zeros((R, V), np.uint32)
    out = dict(idx=np.full((R, S), -1, np.int64), prob=np.zeros((R, S), dt), align=np.zeros((R, S, T), dt),
               length=np.full(R, S, np.int64), raised=np.zeros(R, bool), nan0=np.zeros((R, S), bool), all_nan=np.zeros((R, S), bool))
    done = np.zeros(R, bool)
    for s in range(S):
        scores, states = m.step(target, attended, states, u=u)
        for r in range(R):
            if done[r]:
                continue
            k, p, nan0, all_nan = pick(scores[r], mode, rules)
            out['idx'][r, s], out['prob'][r, s], out['align'][r, s] = k, p, states[-1][r]
            out['nan0'][r, s], out['all_nan'][r, s] = nan0, all_nan
            if nan0:
                scores[r, 0] = np.nan
            if mode == 1 and (all_nan or k == 1):
                out['length'][r], out['raised'][r], done[r] = s + 1, all_nan, True
        if done.all():
            break
        target = scores
    return out


def greedy(m, enc, mode, rules=()):
    """Mode 0: decode_batch_greedy's loop over the whole batch (every row runs its 2T steps; an all-NaN row reports index 1 and NaN
    where numpy would raise).  Mode 1: decode_sequence_greedy's loop, line by line as the reference runs it; a line ends with its
    '\\n', or with `raised` at the step whose candidates are all NaN (reported as index 1 / NaN, as the device marks it).
    -> dict of idx, prob (B, S), align (B, S, T), length, raised (B), nan0, all_nan (B, S); entries behind a line's length are
    idx -1 / 0."""
    if mode == 0:
        return _loop(m, enc, 0, rules)
    B = enc[0].shape[0]
    parts = [_loop(m, [e[j:j + 1] for e in enc], 1, rules) for j in range(B)]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


# ------------------------------------------------------------------------------------------------------------------ cases
def _lines(B, V):
    """B ragged lines of 1-4 characters (the longest has 4 where B > 1); at V = 2 there is no character but the unmapped one."""
    n = [3] if B == 1 else [1 + (3 + 3 * j) % 4 for j in range(B)]
    return [[(2 + (7 * j + 3 * t) % (V - 2)) if V > 2 else 0 for t in range(n[j])] for j in range(B)]


class Case(object):
    """One decode.  family 'uniform' | 'tied'.  sets / gaps / scale: tied_weights.  explicit: decoder states per row
    (explicit_outputs); nan_row: that row's c is NaN.
    Promises (what the CPU test asserts of the fp32 oracle, rows of positive h):
      tie      the indices whose probabilities are bitwise equal and strictly above every other candidate (mode 0's candidates: v >= 1;
               where the set holds index 0 it ties too)
      pick0    the index mode 0 reports at every step            pick1 / len1 / err1   mode 1's first index, length and raise
      neg      (explicit) the indices tied on top in the rows of negative h
      exact    saturated: every probability is exactly 0.0 or 1.0 (the denormal entry apart)"""

    def __init__(self, name, V, B, family='tied', sets=(), gaps=None, scale=1.0, explicit=False, nan_row=None, **promises):
        self.name, self.V, self.B, self.family = name, V, B, family
        self.sets, self.gaps, self.scale, self.explicit, self.nan_row = [tuple(s) for s in sets], dict(gaps or {}), scale, explicit, nan_row
        self.promises = promises
        self.lines = _lines(B, V)
        self.T = max(len(x) for x in self.lines) + 1
        self.S = 2 * self.T
        self.cfg = ModelConfig(depth=DEPTH, width=WIDTH, voc_size=V)
        self.saturated = scale != 1.0
        self.form = greedy_form(V)

    def weights(self, dtype=np.float32):
        w = uniform_weights(self.cfg) if self.family == 'uniform' else tied_weights(self.cfg, self.sets, self.scale, self.gaps)
        return {k: v.astype(dtype) for k, v in w.items()}

    def model(self, dtype=np.float32):
        return OracleModel(self.cfg, self.weights(dtype))

    def texts(self):
        i_c = make_vocabulary(self.V)[1]
        return [''.join(i_c[v] if v else UNMAPPED for v in line) + '\n' for line in self.lines]

    def inputs(self, m):
        """-> (enc_in (B,T,V) as the reference vectorises the lines, idx (B,T) int32 for casv_encode: -1 = padding)"""
        texts = self.texts()
        enc_in, _, _, _ = vectorize_lines(m, texts, [[] for _ in texts])
        idx = np.where(enc_in.any(axis=2), enc_in.argmax(axis=2), -1).astype(np.int32)
        return enc_in, idx

    def encoder_outputs(self, m, nan_row='case'):
        """What the decode starts from: the model's encoder outputs, with the explicit states where the case has them.
        nan_row=None: the same batch with the NaN row finite."""
        enc = m.encode(self.inputs(m)[0])
        if not self.explicit:
            return enc
        return explicit_outputs(enc, self.nan_row if nan_row == 'case' else nan_row)


def run(case, mode, dtype=np.float32, rules=(), nan_row='case'):
    m = case.model(dtype)
    return greedy(m, case.encoder_outputs(m, nan_row), mode, rules)


def _denormal_gap(T):
    """The per-entry amount that puts an entry's logit 95 below the top row's on the saturated model: exp(-95) is a float32 denormal
    (the smallest normal is exp(-87.3), the smallest denormal exp(-103.3))."""
    return 95.0 / (SAT * WIDTH * held_h(T))


def _cases():
    c = []
    # --- uniform: every row is one tie.  Mode 0: index 1 with fl32(1/V) at every step; mode 1: index 0 ties everything, NaN over
    #     p[0], '\n', length 1.  V = 2 leaves a single candidate.
    for V, B in ((2, 3), (12, 1), (40, 37), (255, 3), (256, 17), (257, 3), (640, 17)):
        c.append(Case('u_v%d' % V, V, B, 'uniform', tie=tuple(range(V)), pick0=1, pick1=1, len1=1, err1=False))
    # --- quarter forms: entry v in lane v & 15, slot v >> 4
    for V, B in ((40, 17), (255, 3), (256, 37)):
        for s in ((5, 21), (21, 37), (5, 13), (5, 9), (5, 7), (5, 4), (9, 13), (1, V - 1), (V - 1,), (16, 32, 1), (13, 5, 9)):
            low = min(s)
            c.append(Case('q_v%d_%s' % (V, '_'.join(map(str, s))), V, B, sets=[s], tie=tuple(sorted(s)), pick0=low, pick1=low,
                          len1=1 if low == 1 else None, err1=False))
    # --- whole-wave form (and, at every V, the per-step kernel): entry v in lane v & 63, pass v >> 6
    for V, B in ((257, 3), (640, 37)):
        sets = [(5, 69), (5, 37), (5, 21), (5, 6), (1, V - 1)] + ([(256,)] if V == 257 else [(69, 581)])
        for s in sets:
            low = min(s)
            c.append(Case('w_v%d_%s' % (V, '_'.join(map(str, s))), V, B, sets=[s], tie=tuple(sorted(s)), pick0=low, pick1=low,
                          len1=1 if low == 1 else None, err1=False))
    # the per-step kernel strides by 64 at V = 40 too: the wave sets that fit (the quarter sets at V = 640 are among those above)
    c.append(Case('q_v40_5_37', 40, 3, sets=[(5, 37)], tie=(5, 37), pick0=5, pick1=5, len1=None, err1=False))
    c.append(Case('q_v40_5_6', 40, 1, sets=[(5, 6)], tie=(5, 6), pick0=5, pick1=5, len1=None, err1=False))
    c.append(Case('w_v640_5_13', 640, 3, sets=[(5, 13)], tie=(5, 13), pick0=5, pick1=5, len1=None, err1=False))
    c.append(Case('w_v640_13_5_9', 640, 1, sets=[(13, 5, 9)], tie=(5, 9, 13), pick0=5, pick1=5, len1=None, err1=False))
    # --- the index-0 rule
    for V, B in ((40, 3), (256, 17), (640, 3)):
        for k in (7, 16):
            # index 0 tied with the best entry k: NaN is written, k is picked, the next step is all NaN: mode 1 raises with length 2
            c.append(Case('z_v%d_tie%d' % (V, k), V, B, sets=[(0, k)], tie=(0, k), pick0=k, pick1=k, len1=2, err1=True))
        # index 0 strictly above 7: as the tie
        c.append(Case('z_v%d_above' % V, V, B, sets=[(0,)], gaps={7: GAP}, strict=(0, 7), pick0=7, pick1=7, len1=2, err1=True))
        # index 0 strictly below 7: no NaN, the line runs its 2T steps
        c.append(Case('z_v%d_below' % V, V, B, sets=[(7,)], gaps={0: GAP}, strict=(7, 0), pick0=7, pick1=7, len1=None, err1=False))
        # index 0 tied with '\n': the line ends at step 1, no error
        c.append(Case('z_v%d_newline' % V, V, B, sets=[(0, 1)], tie=(0, 1), pick0=1, pick1=1, len1=1, err1=False))
    # --- saturated: E x 64
    for V, B in ((40, 3), (256, 3), (640, 17)):
        c.append(Case('s_v%d_top7' % V, V, B, sets=[(7,)], scale=SAT, exact=True, pick0=7, pick1=7, len1=None, err1=False))
        c.append(Case('s_v%d_top0' % V, V, B, sets=[(0,)], scale=SAT, exact=True, pick0=1, pick1=1, len1=1, err1=False))
    # one denormal entry: top at index 0, index 21 about 95 below, everything else exactly 0: mode 0 picks 21 (a flush to zero: 1)
    for V, B in ((40, 3), (256, 3), (640, 3)):
        c.append(Case('s_v%d_denormal' % V, V, B, sets=[(0,)], gaps={21: _denormal_gap(5)}, scale=SAT, exact=True, denormal=21,
                      pick0=21, pick1=21, len1=2, err1=True))
    # --- per-row variation: explicit decoder states, set 1 on top in the rows of negative h
    for V, B in ((40, 37), (256, 37), (640, 37), (255, 17), (257, 3)):
        c.append(Case('x_v%d_b%d' % (V, B), V, B, sets=[(5, 21), (9, 13)], explicit=True, tie=(5, 21), neg=(9, 13), pick0=5, pick1=5,
                      len1=None, err1=False))
    c.append(Case('x_v256_zero', 256, 37, sets=[(0, 16), (1, 33)], explicit=True, tie=(0, 16), neg=(1, 33), pick0=16, pick1=16, len1=2,
                  err1=True))
    # --- one all-NaN row between finite ones: row 5 of 37 (inside a quarter-wave group of 4 and a 16-row block), row 1 of 3
    for V, B, r in ((40, 37, 5), (256, 37, 5), (640, 37, 5), (40, 3, 1), (640, 3, 1)):
        c.append(Case('n_v%d_b%d' % (V, B), V, B, sets=[(5, 21), (9, 13)], explicit=True, nan_row=r, tie=(5, 21), neg=(9, 13), pick0=5,
                      pick1=5, len1=None, err1=False))
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
MODES = (0, 1)
